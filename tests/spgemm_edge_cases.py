"""The cases of tests/test_gpu_spgemm_edges.py: k-mer matrices handed over as triples (Engine.set_kmer_matrix) whose rows sit ON the constants of the
overlap SpGEMM (csrc/spgemm.hip, spgemm_direct.hpp, spgemm_table.hpp, ov_plan.hpp) and of the build of A (csrc/matrix.hip).  numpy only.

Every builder returns a Case: (M, N, rows, cols, vals) plus `claims`, what the case says about itself BY CONSTRUCTION — per hub row its owned partners
under the ownership rule, the width of its row of B after the prune and the mirror images it receives; the longest column, the largest position, the
rows of B in 1025 .. 4096 and beyond.  tests/test_spgemm_edge_cases_cpu.py proves every claim with the oracle alone, before a GPU test leans on it.

What the builders know from the code:
  * ownership (spgemm_direct.hpp: owns_pair): row i accumulates the pair {i, j} when i + j is even and j > i, or i + j is odd and j < i; the other row
    receives the mirror image of a surviving pair.  In the dense family (some column of more than 16 entries, positions below 65536) the smaller row owns.
  * a partner claims a table slot with ONE shared column; it survives the prune (numshared >= 2) only with two.
  * the diagonal entry of a row survives when the row has two entries or more.
  * a cold call estimates max(64, entries of the row / 4) distinct partners and never starts a row above the tier guaranteed to fit
    min(entries x longest column, M) partners at load 1/2; option "tune7" = t + 1 starts every row on tier t at least.
The tier limits themselves are NOT stated here: a GPU test reads them from the engine ("overlap_tier_limit_t"), TIER_LIMITS below restates them for the
CPU tests only (hostcpp/test_ov_plan.cpp holds the same literals against plan_ov)."""
import functools

import numpy as np

LDS_TBITS0, NUM_LDS_TIERS = 9, 5
SLAB_PAD = 16
FIN_WAVE_MAX, FIN_WAVE2_MAX, FIN_LDS_MAX = 256, 1024, 4096
RP_TILE = 1024
# family -> the claimed slots at which a row abandons tier 0 .. 4: min(3T/4, T - block) - 1 from the (block, tbits) pairs of OV_ROWS
TIER_LIMITS = {
    "s32": (383, 767, 1535, 3071, 6143),
    "pay": (383, 767, 1535, 3071, 6143),
    "pay16": (383, 767, 1535, 3071, 6143),
    "dense0": (255, 767, 1535, 3071, 6143),
    "dense1": (255, 511, 1535, 3071, 6143),
    "dense2": (255, 511, 1023, 3071, 6143),
}
TIER_BLOCKS = {      # (block, tbits) per tier, as OV_ROWS states them
    "s32": ((128, 9), (256, 10), (512, 11), (1024, 12), (256, 13)),
    "pay": ((128, 9), (256, 10), (512, 11), (1024, 12), (256, 13)),
    "pay16": ((128, 9), (256, 10), (512, 11), (1024, 12), (256, 13)),
    "dense0": ((256, 9), (256, 10), (512, 11), (1024, 12), (256, 13)),
    "dense1": ((256, 9), (512, 10), (512, 11), (1024, 12), (256, 13)),
    "dense2": ((256, 9), (512, 10), (1024, 11), (1024, 12), (256, 13)),
}
OV_DENSE, OV_PAY, OV_S32 = 0, 1, 2
# family -> (engine options set before the matrix, the "overlap_family" / "overlap_pay16" / "overlap_rec16" it must report)
FAMILIES = {
    "s32": ({}, OV_S32, 0, 0),              # positions >= 65536: look-ups, 32-byte records
    "pay": ({"tune3": 1}, OV_PAY, 0, 1),    # a pos16 matrix kept on the 64-bit accumulators
    "pay16": ({}, OV_S32, 1, 1),
    "dense0": ({"dense_up": 0}, OV_DENSE, 0, 1),
    "dense1": ({}, OV_DENSE, 0, 1),
    "dense2": ({"dense_up": 2}, OV_DENSE, 0, 1),
}


def owns(i, j, dense=False):
    """does row i accumulate the pair {i, j}? (arrays allowed)"""
    i, j = np.asarray(i, np.int64), np.asarray(j, np.int64)
    if dense:
        return j > i
    return np.where(((i ^ j) & 1) != 0, j < i, j > i)


class Case:
    def __init__(self, name, M, N, rows, cols, vals, claims, options=None):
        self.name, self.M, self.N = name, int(M), int(N)
        self.rows, self.cols, self.vals = np.asarray(rows, np.int64), np.asarray(cols, np.int64), np.asarray(vals, np.uint32)
        self.claims, self.options = claims, dict(options or {})

    @property
    def triples(self):
        return self.M, self.N, self.rows, self.cols, self.vals


class _Mat:
    """columns one after the other; positions are drawn when the matrix is finished (entry order: column by column)"""

    def __init__(self, M, seed):
        self.M, self.rng, self.r, self.c, self.ncol = int(M), np.random.default_rng(seed), [], [], 0

    def columns(self, members):
        """members: (ncolumns, L) rows, distinct within a column"""
        members = np.asarray(members, np.int64)
        n, L = members.shape
        assert n == 0 or (members.min() >= 0 and members.max() < self.M)
        self.r.append(members.ravel()); self.c.append(np.repeat(np.arange(self.ncol, self.ncol + n), L)); self.ncol += n

    def star(self, hub, partners, shared=1, group=1):
        """columns {hub} + `group` partners each, every one `shared` times: hub and partner share `shared` columns, partners of one column too"""
        partners = np.asarray(partners, np.int64)
        assert hub not in partners and len(np.unique(partners)) == len(partners)
        full = len(partners) // group * group
        for _ in range(shared):
            if full:
                self.columns(np.concatenate([np.full((full // group, 1), hub), partners[:full].reshape(-1, group)], axis=1))
            if full < len(partners):
                self.columns(np.concatenate([[hub], partners[full:]])[None, :])

    def finish(self, pos_lo, pos_hi, pin=None):
        """positions uniform in [pos_lo, pos_hi); pin: (entry, position) pairs set afterwards"""
        rows, cols = np.concatenate(self.r), np.concatenate(self.c)
        vals = self.rng.integers(pos_lo, pos_hi, len(rows)).astype(np.uint32)
        for z, v in (pin or ()):
            vals[z] = v
        return self.M, self.ncol, rows, cols, vals


def _spread(M, n, skip):
    """n ids spread evenly over [0, M), first 0-side and last M - 1 when they are free, none of `skip`"""
    free = np.setdiff1d(np.arange(M), np.asarray(sorted(skip), np.int64))
    assert n <= len(free)
    return free[(np.arange(n) * (len(free) - 1)) // (n - 1)] if n > 1 else free[:n]


def _consecutive(M, n, skip, start):
    free = np.setdiff1d(np.arange(M), np.asarray(sorted(skip), np.int64))
    a = int(np.searchsorted(free, start))
    a = min(a, len(free) - n)
    return free[a:a + n]


def _ends(M, n, skip):
    free = np.setdiff1d(np.arange(M), np.asarray(sorted(skip), np.int64))
    lo = (n + 1) // 2
    return np.concatenate([free[:lo], free[len(free) - (n - lo):]]) if n - lo > 0 else free[:lo]


# ---- a. tier limits -------------------------------------------------------------------------------------------------------------------------------
def _family_shape(family):
    """(dense, column group, position range) that puts a matrix into the family"""
    if family.startswith("dense"):
        return True, 16, (0, 60000)        # columns of 17 reads, positions below 65536
    if family == "s32":
        return False, 3, (0, 200000)       # some position >= 65536 (pinned below)
    return False, 3, (0, 60000)


@functools.lru_cache(maxsize=None)
def tier_case(family, tier, owned, placed="tune7"):
    """Hub row 0 with exactly `owned` owned partners — each through ONE shared column but the first 40, which survive the prune —, 30 partners it does
    not own (general families), and the partners' own short rows on the same tier.  placed = "tune7": option tune7 = tier + 1 starts every row on `tier`;
    "estimate": the hub has just enough entries (padding columns {0, x} that repeat partners) that the cold estimate alone starts it on `tier`."""
    dense, group, (plo, phi) = _family_shape(family)
    M = 2 * owned + 200
    m = _Mat(M, 1000 + 17 * tier + owned)
    hub = 0
    mine = np.arange(1, owned + 1) if dense else 2 * np.arange(1, owned + 1)      # owned by row 0: every larger row (dense) | the even ones
    surv = min(40, owned)
    m.star(hub, mine[:surv], shared=2, group=group)
    m.star(hub, mine[surv:], shared=1, group=group)
    theirs = np.zeros(0, np.int64) if dense else 2 * np.arange(30) + 1
    if len(theirs):
        m.star(hub, theirs, shared=2, group=group)
    width = 1 + surv + len(theirs)
    images = len(theirs)
    entries = 2 * ((surv + group - 1) // group) + (owned - surv + group - 1) // group + 2 * ((len(theirs) + group - 1) // group)
    options = dict(FAMILIES[family][0])
    if placed == "tune7":
        options["tune7"] = tier + 1
    else:
        lim = TIER_LIMITS[family]
        lo = 4 * (lim[tier - 1] + 1) if tier > 0 else 0      # est = entries / 4 (>= 64) must pass limit[tier - 1] and stay within limit[tier]
        want = max(lo + 8, entries)
        assert want // 4 <= lim[tier], (want, lim[tier])
        pad = mine[np.arange(want - entries) % len(mine)]
        m.columns(np.stack([np.full(len(pad), hub), pad], axis=1))
        entries = want
        width = 1 + len(np.unique(np.concatenate([mine[:surv], pad]))) + len(theirs)      # (a partner of the padding shares two columns or more with the hub: it survives)
    pin = [(0, 70000)] if family == "s32" else None
    Mx, N, rows, cols, vals = m.finish(plo, phi, pin)
    claims = {"family": family, "tier": tier, "placed": placed, "dense": dense,
              "hubs": {hub: {"owned": owned, "width": width, "images": images, "entries": entries}},
              "max_col": group + 1, "pos16": family != "s32", "other_rows_owned_max": group + 1}
    return Case("tier_%s_t%d_%d_%s" % (family, tier, owned, placed), Mx, N, rows, cols, vals, claims, options)


@functools.lru_cache(maxsize=None)
def guaranteed_case(tier, above, pos16):
    """guaranteed_tbits switches at need = T/2 | T/2 + 1: M = T/2 (+ 1 with `above`) rows, hub row 0 with so many entries that the cold estimate asks for
    tier + 1 — k_classify_direct starts it on `tier`, the tier guaranteed to fit M partners, and on tier + 1 (5: the HBM tables) with one row more."""
    T = 1 << (LDS_TBITS0 + tier)
    M = T // 2 + (1 if above else 0)
    lim = TIER_LIMITS["s32"][tier]
    entries = 4 * (lim + 1) + 8
    m = _Mat(M, 2000 + tier)
    partners = np.arange(1, M)
    m.star(0, partners, shared=1, group=3)
    have = (len(partners) + 2) // 3
    pad = partners[np.arange(entries - have) % len(partners)]
    m.columns(np.stack([np.zeros(len(pad), np.int64), pad], axis=1))
    Mx, N, rows, cols, vals = m.finish(0, 60000 if pos16 else 200000, None if pos16 else [(0, 70000)])
    npad = np.bincount(pad, minlength=M)
    width = 1 + int((npad[1:] + 1 >= 2).sum())
    claims = {"tier": tier, "above": above, "dense": False, "pos16": pos16, "max_col": 4,
              "hubs": {0: {"owned": int(owns(0, partners).sum()), "width": width, "images": int((~owns(0, partners) & (npad[1:] + 1 >= 2)).sum()), "entries": entries}}}
    return Case("guaranteed_t%d_%s_%s" % (tier, "above" if above else "at", "pos16" if pos16 else "pos32"), Mx, N, rows, cols, vals, claims, {})


# ---- b. finalize widths ---------------------------------------------------------------------------------------------------------------------------
WIDTHS = (1, 2, 63, 64, 65, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 2047, 4095, 4096, 4097, 8193)
FORMATS = {"rec16": ({}, (0, 60000), 1), "mir32": ({"mir32": 1}, (0, 60000), 0), "pos32": ({}, (0, 200000), 0)}      # options, positions, "overlap_rec16"


@functools.lru_cache(maxsize=None)
def widths_case(layout, fmt):
    """One hub row per width of WIDTHS: w - 1 partners through two columns {hub, partner} each + the diagonal (width 1: two partners through ONE column
    each).  Hubs are no partners of each other.  layout "spread": partners evenly over [0, M), hubs 0 and M - 1 among the hubs; "consecutive": a run of
    neighbouring ids (a dozen buckets or more of the bucket sorts — a bucket holds 8 M / width columns —; ONE bucket: one_bucket_case); "ends": half at 0 .., half at .. M - 1 (rows 0 and M - 1 are partners, the hubs sit inside)."""
    M = 12000
    m = _Mat(M, 3000 + len(layout))
    if layout == "ends":
        hubs = 300 + 601 * np.arange(len(WIDTHS))
    else:
        hubs = np.concatenate([[0], 311 + 607 * np.arange(len(WIDTHS) - 2), [M - 1]])
    order = np.random.default_rng(5).permutation(len(WIDTHS))      # (which width sits on which hub: rows 0 and M - 1 get what the shuffle gives them)
    skip = set(int(h) for h in hubs)
    claim_hubs = {}
    for k, w in enumerate(WIDTHS):
        h = int(hubs[order[k]])
        n = max(w - 1, 0)
        if layout == "spread":
            p = _spread(M, n, skip)
        elif layout == "consecutive":
            p = _consecutive(M, n, skip, (h * 7 + 1000) % (M - n - 40))
        else:
            p = _ends(M, n, skip)
        assert len(p) == n
        if w == 1:
            q = _consecutive(M, 2, skip, 5000)
            m.star(h, q, shared=1)
            claim_hubs[h] = {"width": 1, "owned": int(owns(h, q).sum()), "images": 0, "entries": 2}
        else:
            m.star(h, p, shared=2)
            claim_hubs[h] = {"width": w, "owned": int(owns(h, p).sum()), "images": int((~owns(h, p)).sum()), "entries": 2 * n}
    opts, (plo, phi), rec16 = FORMATS[fmt]
    Mx, N, rows, cols, vals = m.finish(plo, phi, [(0, 70000)] if fmt == "pos32" else None)
    claims = {"hubs": claim_hubs, "max_col": 2, "pos16": fmt != "pos32", "rec16": rec16, "dense": False,
              "sort_rows": (sum(1 for w in WIDTHS if FIN_WAVE2_MAX < w <= FIN_LDS_MAX), sum(1 for w in WIDTHS if w > FIN_LDS_MAX)),
              "partner_width_max": 1 + len(WIDTHS)}
    return Case("widths_%s_%s" % (layout, fmt), Mx, N, rows, cols, vals, claims, opts)


@functools.lru_cache(maxsize=None)
def numshared_case():
    """A 600-wide row (k_finalize_mid16's range, 16-byte records) two of whose pairs — one it owns, one it receives — share 40 000 columns each: its numshared word is large where the
    kernel keeps a record's place in bits 22 .. 31 of it."""
    M, big = 3000, 40000
    m = _Mat(M, 4000)
    h, x, y = 1000, 2001, 1500       # h + x odd, x > h: x owns {h, x} — h receives the image; h + y even, y > h: h owns {h, y} and mirrors it
    p = _spread(M, 597, {h, x, y})
    m.star(h, p, shared=2)
    m.columns(np.tile([[h, x]], (big, 1)))
    m.columns(np.tile([[h, y]], (big, 1)))
    Mx, N, rows, cols, vals = m.finish(0, 60000)
    claims = {"hubs": {h: {"width": 600, "owned": int(owns(h, p).sum()) + 1, "images": int((~owns(h, p)).sum()) + 1, "entries": 2 * 597 + 2 * big}},
              "max_col": 2, "pos16": True, "dense": False, "max_numshared": 2 * big + 2 * 597, "pair_numshared": {(h, x): big, (h, y): big}, "sort_rows": (0, 0)}
    return Case("numshared", Mx, N, rows, cols, vals, claims, {})


# ---- c. mirror slabs ------------------------------------------------------------------------------------------------------------------------------
IMAGES = (0, 1, 15, 16, 17, 40, 300)


@functools.lru_cache(maxsize=None)
def slab_case():
    """Rows 1000 .. 1006 receive exactly IMAGES[k] mirror images — from partners beyond 1100 of the other parity, which own the pair — and stage three
    entries of their own (partners below 900 of the other parity).  Z < 65536: with "slab_q16" = 1 every slab is exactly SLAB_PAD entries."""
    M = 3000
    m = _Mat(M, 5000)
    hubs = {}
    for k, n in enumerate(IMAGES):
        r = 1000 + k
        senders = 1101 + (r & 1) + 2 * np.arange(n) + 2 * 7 * k      # r + x odd, x > r: x owns
        mine = 101 + (r & 1) + 2 * np.arange(3) + 10 * k            # r + x odd, x < r: r owns
        assert not owns(r, senders).any() and owns(r, mine).all()
        if n:
            m.star(r, senders, shared=2)
        m.star(r, mine, shared=2)
        hubs[r] = {"width": 1 + n + 3, "owned": 3, "images": n, "entries": 2 * (n + 3)}
    Mx, N, rows, cols, vals = m.finish(0, 60000)
    assert len(rows) < 65536
    claims = {"hubs": hubs, "max_col": 2, "pos16": True, "dense": False}
    return Case("slabs", Mx, N, rows, cols, vals, claims, {})


def slab_sizes(a_rowptr, q16):
    """entries of every row's slab at ratio q16 (spgemm.hip: slab_base): floor(rp[j + 1] q >> 16) - floor(rp[j] q >> 16) + SLAB_PAD"""
    rp = np.asarray(a_rowptr, np.int64) - int(a_rowptr[0])
    base = (rp * int(q16)) >> 16
    return np.diff(base) + SLAB_PAD


# ---- d. row pointers ------------------------------------------------------------------------------------------------------------------------------
ROWPTR_M = (1023, 1024, 1025, 2047, 2048, 2049, 131071, 131072, 131073)


@functools.lru_cache(maxsize=None)
def rowptr_case(M):
    """A few thousand entries among a few hundred rows of M; rows 0, 1023 (M > 1023), 1024 (M > 1024) and M - 1 hold entries; row M - 1, in the last
    tile of k_row_pointers, is as wide as M allows up to 1101 entries."""
    m = _Mat(M, 6000 + M % 1000)
    rng = np.random.default_rng(M)
    wide = M - 1
    marks = sorted({0, min(1023, M - 1), min(1024, M - 1), M - 1} - {wide})
    n = min(1100, M - 16)
    skip = set(marks) | {wide}
    # (partners of the wide row: the last tile's own rows first, then rows spread over the matrix)
    near = _consecutive(M, min(n, 300), skip, max(M - 700, 0))
    far = _spread(M, n - len(near), skip | set(int(x) for x in near))
    p = np.concatenate([near, far])
    m.star(wide, p, shared=2)
    hubs = {wide: {"width": 1 + n, "owned": int(owns(wide, p).sum()), "images": int((~owns(wide, p)).sum()), "entries": 2 * n}}
    for r in marks:      # the marked rows: a pair of their own each, with a row nobody else uses
        free = np.setdiff1d(np.arange(M), np.concatenate([p, [wide], marks]))
        q = int(free[rng.integers(0, len(free))])
        m.star(r, [q], shared=2)
        skip.add(q)
        hubs[r] = {"width": 2, "owned": int(owns(r, q)), "images": int(not owns(r, q)), "entries": 2}
        p = np.concatenate([p, [q]])
    Mx, N, rows, cols, vals = m.finish(0, 60000)
    claims = {"hubs": hubs, "max_col": 2, "pos16": True, "dense": False, "sort_rows": (1 if 1 + n > FIN_WAVE2_MAX else 0, 0), "scan": M + 1 > (1 << 17)}
    return Case("rowptr_%d" % M, Mx, N, rows, cols, vals, claims, {})


# ---- e. shape switches of A ---------------------------------------------------------------------------------------------------------------------------
def _background(m, nrows, ncols, lo):
    """ncols columns of two or three rows among rows lo .. lo + nrows - 1, every column twice (pairs survive)"""
    rng = m.rng
    for L in (2, 3):
        mem = np.stack([rng.choice(nrows, L, replace=False) + lo for _ in range(ncols // 2)])
        m.columns(mem); m.columns(mem)


@functools.lru_cache(maxsize=None)
def column_case(longest):
    """the longest column holds `longest` rows (twice: its pairs survive); 4 | 5: stride 4 -> 8, fbits 2 -> 3; 16 | 17: general -> dense path;
    32 | 33: the dense path's partner blocks of 32 -> 64; 64 | 65: padded columns -> CSC.  The matrix of L + 1 is the matrix of L plus ONE entry per copy."""
    M = 600
    m = _Mat(M, 7000)
    _background(m, 400, 300, 100)
    big = np.arange(0, 2 * 66, 2)[:longest][None, :] + 1       # odd rows 1, 3, ...: the first `longest` of a fixed list
    m.columns(big)
    Mx, N, rows, cols, vals = m.finish(0, 60000)
    # (the second copy last, so that the matrices of L and L + 1 draw the same positions for their common entries but one)
    rows = np.concatenate([rows, big.ravel()]); cols = np.concatenate([cols, np.full(longest, N)]); vals = np.concatenate([vals, (np.arange(longest) * 37 + 11).astype(np.uint32)]); N += 1
    stride = 0 if longest > 64 else (4 if longest <= 4 else (longest + 7) & ~7)
    fbits = 2 if stride else 1
    while (stride and (1 << fbits) < stride) or (not stride and (longest - 1) >> fbits):
        fbits += 1
    claims = {"max_col": longest, "pos16": True, "dense": longest > 16 and longest <= 64, "stride": stride, "fbits": fbits,
              "suffix": 1 if 16 < longest <= 64 else 0, "hubs": {}}
    return Case("column_%d" % longest, Mx, N, rows, cols, vals, claims, {})


@functools.lru_cache(maxsize=None)
def position_case(largest):
    """the largest position is `largest`: 65535 | 65536 (pos16: 16-byte records, payload accumulators, inline partners), 2^30 - 1 | 2^30 (ownership hints).
    The entry that carries it belongs to a surviving pair."""
    M = 600
    m = _Mat(M, 7100)
    _background(m, 400, 300, 100)
    Mx, N, rows, cols, vals = m.finish(0, 50000, [(3, largest)])
    claims = {"max_col": 3, "max_pos": largest, "pos16": largest < 65536, "hints": 1 if largest < (1 << 30) else 0, "dense": False, "hubs": {}}
    return Case("position_%d" % largest, Mx, N, rows, cols, vals, claims, {})


def bits_for(x):
    return max(int(x).bit_length(), 1)


@functools.lru_cache(maxsize=None)
def csr_words_case(over):
    """mb + nb + pb + 2 = 64 | 65: 131072 rows (17 bits), positions up to 2^32 - 1 (32 bits), 8192 | 8193 columns (13 | 14 bits) — the matrix of 65 is
    the matrix of 64 plus one column of two entries."""
    M, N0 = 131072, 8192
    m = _Mat(M, 7200)
    rng = m.rng
    hot = np.unique(np.concatenate([[0, M - 1], rng.choice(M, 500, replace=False)]))
    mem = np.stack([rng.choice(hot, 2, replace=False) for _ in range(N0 // 2)])
    m.columns(mem); m.columns(mem)
    if over:
        m.columns(mem[:1])
    Mx, N, rows, cols, vals = m.finish(0, 1 << 32, [(5, (1 << 32) - 1)])
    bits = bits_for(M - 1) + bits_for(N - 1) + 32 + 2
    assert bits == (65 if over else 64)
    claims = {"max_col": 2, "pos16": False, "hints": 0, "csr_words": 0 if over else 1, "bits": bits, "dense": False, "hubs": {}}
    return Case("csr_words_%d" % bits, Mx, N, rows, cols, vals, claims, {})


@functools.lru_cache(maxsize=None)
def pay16_case(stride, entries):
    """max_row_nnz << fbits = 65536 | 65537 + : row 0 holds `entries` entries (16384 | 16385 at stride 4, fbits 2; 8192 | 8193 at stride 8, fbits 3).  Its
    LAST 400 entries — the highest column ids — are 200 surviving pairs (100 owned by row 0, 100 not); a product sequence number cut to 16 bits would name
    another entry's position in their seeds."""
    M = 9000
    m = _Mat(M, 7300 + stride)
    hub = 0
    last_even, last_odd = 2 * np.arange(4001, 4101), 2 * np.arange(4001, 4101) + 1
    lone = entries & 1                           # the one entry more: a column that holds row 0 alone
    n1 = entries - 400 - lone
    singles = 1 + np.arange(n1) % 7000          # one shared column each: partners 1 .. 7000 (repeats share two)
    if stride == 8:                              # one column of five rows that row 0 is no member of
        m.columns(np.array([[8900, 8901, 8902, 8903, 8904]])); m.columns(np.array([[8900, 8901, 8902, 8903, 8904]]))
    m.columns(np.stack([np.full(n1, hub), singles], axis=1))
    if lone:
        m.columns(np.array([[hub]]))
    m.star(hub, np.concatenate([last_even, last_odd]), shared=2)
    Mx, N, rows, cols, vals = m.finish(0, 60000)
    fbits = 2 if stride == 4 else 3
    cnt = np.bincount(singles, minlength=M)
    width = 1 + int((cnt >= 2).sum()) + 200
    claims = {"max_col": 2 if stride == 4 else 5, "pos16": True, "dense": False, "stride": stride, "fbits": fbits, "pay16": 1 if (entries << fbits) <= 65536 else 0,
              "hubs": {hub: {"width": width, "entries": entries,
                             "owned": int(owns(hub, np.unique(singles)).sum()) + 100, "images": int((~owns(hub, np.flatnonzero(cnt >= 2))).sum()) + 100}}}
    return Case("pay16_s%d_%d" % (stride, entries), Mx, N, rows, cols, vals, claims, {})


# ---- what the oracle says about a case (tests/test_spgemm_edge_cases_cpu.py) ----------------------------------------------------------------------
def pattern_facts(M, colptr, csc_read, dense):
    """From the columns of A alone: per row the distinct partners it owns under the ownership rule (before the prune) and the mirror images it receives
    (pairs that share two columns or more and are owned by the other row); the longest column."""
    colptr, csc_read = np.asarray(colptr, np.int64), np.asarray(csc_read, np.int64)
    lens = np.diff(colptr)
    keys = []
    for L in np.unique(lens):
        if L < 2:
            continue
        which = np.flatnonzero(lens == L)
        mem = csc_read[colptr[which][:, None] + np.arange(L)[None, :]]
        a, b = np.triu_indices(int(L), 1)
        lo, hi = np.minimum(mem[:, a], mem[:, b]).ravel(), np.maximum(mem[:, a], mem[:, b]).ravel()
        ok = lo != hi
        keys.append(lo[ok] * M + hi[ok])
    owned, images = np.zeros(M, np.int64), np.zeros(M, np.int64)
    if keys:
        k, cnt = np.unique(np.concatenate(keys), return_counts=True)
        lo, hi = k // M, k % M
        lo_owns = owns(lo, hi, dense)
        np.add.at(owned, np.where(lo_owns, lo, hi), 1)
        s = cnt >= 2
        np.add.at(images, np.where(lo_owns, hi, lo)[s], 1)
    return owned, images, int(lens.max()) if len(lens) else 0


# ---- one bucket of the finalize's bucket sorts; one row per tier ------------------------------------------------------------------------------------
FIN_BUCKETS = 512
ONE_BUCKET_M = 1 << 21
ONE_BUCKET_WIDTHS = (300, 1024, 1025, 4096)


def fin_bucket(col, width, M):
    """the bucket k_finalize_mid / _mid16 (257 .. 1024 entries: width / 8 buckets, 128 at most) and k_finalize_bucket (1025 .. 4096: 512 at most) give a
    column of a row of `width` entries: col * floor(nb * 2^32 / M) >> 32"""
    nb = max(min(width // 8, 128 if width <= FIN_WAVE2_MAX else FIN_BUCKETS), 1)
    return (np.asarray(col, np.int64) * ((nb << 32) // M)) >> 32


@functools.lru_cache(maxsize=None)
def one_bucket_case(fmt):
    """Rows whose partners ALL fall into one bucket ("degrades to a rank sort"): that needs M >= buckets x width — a row of y entries has y / 8 buckets of 8 M / y
    columns, at M = 12 000 (widths_case) 94 columns for y = 1025 and 23 for y = 4096.  M = 2^21, mostly empty: a bucket of the 512 of y = 4096 holds 4096
    columns, one of the 128 of y = 1024 | 1025 holds 16 384; hub row 4096 k with the w - 1 rows behind it as partners fills one bucket with w = 300, 1024 (mid), 1025 and 4096 (bucket: exactly full)."""
    M = ONE_BUCKET_M
    m = _Mat(M, 8000)
    hubs = {}
    for k, w in enumerate(ONE_BUCKET_WIDTHS):
        h = 4096 * (37 + 101 * k) if k < 3 else M - 4096      # (the last hub: the last bucket, column M - 1 among its partners)
        p = h + 1 + np.arange(w - 1)
        m.star(h, p, shared=2)
        hubs[h] = {"width": w, "owned": int(owns(h, p).sum()), "images": int((~owns(h, p)).sum()), "entries": 2 * (w - 1)}
    opts, (plo, phi), rec16 = FORMATS[fmt]
    Mx, N, rows, cols, vals = m.finish(plo, phi)
    claims = {"hubs": hubs, "max_col": 2, "pos16": True, "rec16": rec16, "dense": False, "sort_rows": (2, 0), "one_bucket": True}
    return Case("one_bucket_%s" % fmt, Mx, N, rows, cols, vals, claims, opts)


EVERY_TIER_OWNED = (600, 1200, 2400, 4800, 7200)      # more than tiers 0 .. 4 take (383, 767, 1535, 3071, 6143 claims), no more than the next takes


@functools.lru_cache(maxsize=None)
def every_tier_case():
    """Five hub rows 0 .. 4 that can complete only on tiers 1, 2, 3, 4 and on the HBM tables: EVERY_TIER_OWNED owned partners each (rows beyond 100 of the
    hub's own parity, one shared column each but 40 that survive).  Fewer than 2^18 entries: no in-call prediction forwards a row, the cold estimate
    (entries / 4) starts each hub below the tier that fits it and the tiers hand it on."""
    M = 2 * max(EVERY_TIER_OWNED) + 300
    m = _Mat(M, 8100)
    hubs = {}
    for h, n in enumerate(EVERY_TIER_OWNED):
        p = 100 + (h & 1) + 2 * np.arange(n)
        assert owns(h, p).all()
        m.star(h, p[:40], shared=2)
        m.star(h, p[40:], shared=1)
        hubs[h] = {"width": 41, "owned": n, "images": 0, "entries": n + 40}
    Mx, N, rows, cols, vals = m.finish(0, 60000)
    assert len(rows) < (1 << 18)
    claims = {"hubs": hubs, "max_col": 2, "pos16": True, "dense": False, "other_rows_owned_max": 0}
    return Case("every_tier", Mx, N, rows, cols, vals, claims, {})


# ---- the list of cases ----------------------------------------------------------------------------------------------------------------------------------
def tier_counts(tier, limit):
    """owned partners of the hub row around a tier's limit and around half its table"""
    T = 1 << (LDS_TBITS0 + tier)
    return (limit - 1, limit, limit + 1, T // 2, T // 2 + 1)


ESTIMATE_TIER = {"s32": 1, "pay": 2, "pay16": 3, "dense0": 1, "dense1": 2, "dense2": 3}      # the tier of each family's case placed by the cold estimate


DENSE_UP = {"dense0": 0, "dense1": 1, "dense2": 2}      # no row of the dense family starts below tier "dense_up"


def all_cases():
    """every case of the GPU file, with the tier limits as TIER_LIMITS restates them (the GPU tests read them from the engine)"""
    out = []
    for family, lim in TIER_LIMITS.items():
        for t in range(DENSE_UP.get(family, 0), NUM_LDS_TIERS):
            out += [tier_case(family, t, n) for n in tier_counts(t, lim[t])]
        t = ESTIMATE_TIER[family]
        out += [tier_case(family, t, n, "estimate") for n in (lim[t], lim[t] + 1)]
    out += [guaranteed_case(t, above, pos16) for t in range(NUM_LDS_TIERS) for above in (False, True) for pos16 in (True, False)]
    out += [widths_case(layout, fmt) for layout in ("spread", "consecutive", "ends") for fmt in FORMATS]
    out += [numshared_case(), slab_case(), every_tier_case(), one_bucket_case("rec16"), one_bucket_case("mir32")]
    out += [rowptr_case(M) for M in ROWPTR_M]
    out += [column_case(L) for L in (4, 5, 16, 17, 32, 33, 64, 65)]
    out += [position_case(v) for v in (65535, 65536, (1 << 30) - 1, 1 << 30)]
    out += [csr_words_case(False), csr_words_case(True)]
    out += [pay16_case(4, 16384), pay16_case(4, 16385), pay16_case(8, 8192), pay16_case(8, 8193)]
    return out
