"""-m gpu: every device primitive of prims.hip called on its own, through the test-only harness of tests/primcheck, at its own boundaries
(sizes around the tiles and the levels of the scans, every digit split, stability, empty and crowded groups), each result compared in full with
the plain references of tests/prim_util.py.  All comparisons are integer and exact."""
import numpy as np
import pytest

import prim_util as pu

pytestmark = pytest.mark.gpu

TILE = pu.RS_TILE
U64 = np.uint64


def _rng(*seed):
    return np.random.default_rng(list(seed))


def _eq(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    if not (got == want).all():
        bad = np.flatnonzero((got != want).reshape(-1))
        z = int(bad[0])
        raise AssertionError("%s: %d of %d places differ, the first at %d: got %r, want %r" % (what, bad.size, got.size, z, got.reshape(-1)[z], want.reshape(-1)[z]))


# ---- scans -------------------------------------------------------------------------------------------------------------------------------
SCAN_N = (0, 1, 2, 63, 64, 65, 2047, 2048, 2049, 2048 ** 2 - 1, 2048 ** 2, 2048 ** 2 + 1)


def _scan_values(kind, n):
    if kind == "zeros":
        return np.zeros(n, dtype=np.uint32)
    if kind == "ones":
        return np.ones(n, dtype=np.uint32)
    if kind == "random":      # (the sum passes 2^32 from a handful of items on)
        return _rng(1, n).integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    x = _rng(2, n).integers(0, 3, n, dtype=np.uint64).astype(np.uint32)      # "huge": 2^32 - 1 in the last place of a tile in the middle
    if n:
        x[min(n - 1, (n // pu.SCAN_TILE // 2) * pu.SCAN_TILE + pu.SCAN_TILE - 1)] = 0xFFFFFFFF
    return x


@pytest.mark.parametrize("kind", ["zeros", "ones", "random", "huge"])
def test_exclusive_scans(kind):
    for n in SCAN_N:
        x = _scan_values(kind, n)
        exact = pu.exclusive_scan_exact(x)
        if kind == "random" and n >= 63:
            assert int(exact[-1]) > 1 << 32      # the u32 result wraps, the i64 result must not
        _eq(pu.scan_u32(x), (exact & U64(0xFFFFFFFF)).astype(np.uint32), "exclusive_scan_u32 %s n=%d" % (kind, n))
        _eq(pu.scan_u32(x, inplace=True), (exact & U64(0xFFFFFFFF)).astype(np.uint32), "exclusive_scan_u32 in == out %s n=%d" % (kind, n))
        _eq(pu.scan_u32_to_i64(x), exact.astype(np.int64), "exclusive_scan_u32_to_i64 %s n=%d" % (kind, n))


# ---- sorts -------------------------------------------------------------------------------------------------------------------------------
def _bit_ranges(maxbit):
    r = [(lo, lo + w) for lo in (0, 5) for w in range(1, 13)]
    r += [(0, hi) for hi in (17, 18, 19, 27, 28, 34, 36, 37, 45, 46, 63, 64) if hi <= maxbit]
    if maxbit == 64:
        r.append((40, 64))
    else:
        r += [(0, 32), (20, 32)]      # (the 32-bit keys' own upper end)
    return r


SMALL_N = (2, 63, 65, TILE - 1, TILE, TILE + 1, 3 * TILE + 1)
DISTRIBUTIONS = ("uniform", "equal", "dominant", "sorted", "reverse", "outside")


def _keys(dist, n, lo, hi, maxbit, seed):
    """n keys of maxbit bits; the distribution is that of the SORTED field, the bits outside it are random (they ride along)"""
    rng = _rng(seed, n, lo, hi)
    full = (1 << maxbit) - 1
    fmask = ((1 << (hi - lo)) - 1) << lo
    k = rng.integers(0, 1 << 64, n, dtype=np.uint64) & U64(full)
    if dist == "uniform":
        return k
    outside = k & U64(full & ~fmask)
    if dist == "outside":      # keys that differ only outside the sorted bits: the output is the input
        return outside | U64(fmask & 0x5A5A5A5A5A5A5A5A)
    if dist == "equal":        # ONE key: a tile holds one digit only, 8192 times
        return np.full(n, int(k[0]) if n else 0, dtype=np.uint64)
    if dist == "dominant":     # one digit of every pass holds all but a handful
        f = np.full(n, (fmask & 0x3333333333333333), dtype=np.uint64)
        few = rng.integers(0, n, min(n, 5))
        f[few] = k[few] & U64(fmask)
        return outside | f
    order = np.sort(pu.sort_field(k, lo, hi))      # "sorted" / "reverse": the field ascending or descending, with ties where it is narrow
    if dist == "reverse":
        order = order[::-1]
    return outside | (order << U64(lo))


def _check_sort(kind, keys, lo, hi, what):
    n = keys.size
    vals = np.arange(n, dtype=np.uint64)      # the input index: stability is visible
    k32 = kind == "pairs_k32"
    kin = keys.astype(np.uint32) if k32 else keys
    if kind == "keys":
        where, k0, k1 = pu.sort_keys(kin, lo, hi)
        bufs = [(k0,), (k1,)]
        before = [(kin,), (np.full(n, pu.OTHER_KEY, dtype=np.uint64),)]
    else:
        where, b0, b1 = pu.sort_pairs(kin, vals, lo, hi, k32=k32)
        bufs = [b0, b1]
        before = [(kin, vals), (np.full(n, pu.OTHER_KEY & (0xFFFFFFFF if k32 else (1 << 64) - 1), dtype=kin.dtype), np.full(n, pu.OTHER_VAL, dtype=np.uint64))]
    assert where == pu.sort_where(n, lo, hi) == pu.sort_where_ref(n, lo, hi), (what, where)
    if n <= 1 or hi <= lo:      # nothing runs: both buffers as they were
        assert where == 0
        for got, want in zip(bufs, before):
            for g, w in zip(got, want):
                _eq(g, w, what + " (left alone)")
        return
    order = pu.stable_order(kin, lo, hi)
    _eq(bufs[where][0], kin[order], what + " keys")
    if kind != "keys":
        _eq(bufs[where][1], vals[order], what + " values (stability)")


@pytest.mark.parametrize("dist", DISTRIBUTIONS)
@pytest.mark.parametrize("kind", ["pairs", "keys", "pairs_k32"])
def test_radix_sorts_every_digit_split_around_the_tiles(kind, dist):
    maxbit = 32 if kind == "pairs_k32" else 64
    for lo, hi in _bit_ranges(maxbit):
        for n in SMALL_N:
            _check_sort(kind, _keys(dist, n, lo, hi, maxbit, 11), lo, hi, "%s %s n=%d bits [%d, %d)" % (kind, dist, n, lo, hi))


@pytest.mark.parametrize("kind", ["pairs", "keys", "pairs_k32"])
def test_radix_sorts_that_do_not_run_leave_both_buffers(kind):
    maxbit = 32 if kind == "pairs_k32" else 64
    for n, lo, hi in ((0, 0, maxbit), (1, 0, maxbit), (1, 5, 6), (100, 7, 7), (100, 9, 3), (TILE + 1, 20, 20)):
        _check_sort(kind, _keys("uniform", n, 0, maxbit, maxbit, 12), lo, hi, "%s n=%d bits [%d, %d)" % (kind, n, lo, hi))


def test_last_partial_tile_of_one_key_and_one_digit_tiles():
    """stability as such: 8192 equal keys per tile is the worst case of the scatter's 16-bit per-wavefront counters; a last tile of ONE key"""
    for kind in ("pairs", "keys", "pairs_k32"):
        for n in (TILE + 1, 3 * TILE + 1):
            for lo, hi in ((0, 9), (3, 4), (0, 18), (0, 32)):
                keys = np.full(n, 0x00000000F0F0F0F0 if kind == "pairs_k32" else 0xF0F0F0F0F0F0F0F0, dtype=np.uint64)
                keys[-1] = 0      # the smallest key sits alone in the last tile and must come out first
                _check_sort(kind, keys, lo, hi, "%s one digit per tile n=%d bits [%d, %d)" % (kind, n, lo, hi))


MID_N = (256 * TILE, 256 * TILE + 1)      # 256 tiles: the last size of the one-workgroup column scan, and the first of two levels
BIG_N = 30 * 1000 * 1000 + 11             # 3663 tiles: two levels of the column scan


@pytest.mark.parametrize("kind", ["pairs", "keys", "pairs_k32"])
def test_radix_sorts_at_the_column_scans_levels(kind):
    maxbit = 32 if kind == "pairs_k32" else 64
    for n in MID_N:
        for dist, lo, hi in (("uniform", 0, maxbit), ("dominant", 5, 17), ("equal", 0, 9), ("uniform", maxbit - 24, maxbit), ("outside", 5, 6), ("reverse", 0, 10)):
            _check_sort(kind, _keys(dist, n, lo, hi, maxbit, 13), lo, hi, "%s %s n=%d bits [%d, %d)" % (kind, dist, n, lo, hi))


@pytest.mark.parametrize("kind,dist,lo,hi", [("pairs", "uniform", 0, 64), ("keys", "dominant", 40, 64), ("pairs_k32", "uniform", 0, 32)])
def test_radix_sorts_of_tens_of_millions(kind, dist, lo, hi):
    """the largest case of this file: 3 * 10^7 pairs = four buffers of 240 MB + 8 MB of histograms on the device"""
    maxbit = 32 if kind == "pairs_k32" else 64
    _check_sort(kind, _keys(dist, BIG_N, lo, hi, maxbit, 14), lo, hi, "%s %s n=%d bits [%d, %d)" % (kind, dist, BIG_N, lo, hi))


# ---- the first histogram handed over ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lo,hi", [(0, 34), (0, 9), (5, 6), (40, 64), (0, 64), (3, 21)])
def test_first_histogram_handed_over(lo, hi):
    for n in (2, TILE - 1, TILE, TILE + 1, 3 * TILE + 1, 256 * TILE + 1):
        for dist in ("uniform", "dominant"):
            keys = _keys(dist, n, lo, hi, 64, 15)
            shift, bits, tile, offset = pu.first_histogram_layout(n, lo, hi)
            assert (shift, bits) == pu.radix_digits(lo, hi)[0] and tile == TILE and offset == 0
            # what a producer does while it writes the keys: row t = the digit counts of the keys [t * tile, (t + 1) * tile)
            nrows = (n + tile - 1) // tile
            digit = ((keys >> U64(shift)) & U64((1 << bits) - 1)).astype(np.int64)
            counts = np.bincount(np.arange(n) // tile * (1 << bits) + digit, minlength=nrows << bits).astype(np.uint32).reshape(nrows, 1 << bits)
            want = keys[pu.stable_order(keys, lo, hi)]
            what = "%s n=%d bits [%d, %d)" % (dist, n, lo, hi)
            w1, a0, a1 = pu.sort_keys_first_hist(keys, lo, hi, counts)
            w0, b0, b1 = pu.sort_keys(keys, lo, hi)
            assert w0 == w1 == pu.sort_where_ref(n, lo, hi)
            _eq((a0, a1)[w1], want, "first histogram handed over " + what)
            _eq((b0, b1)[w0], want, "first histogram counted by the sort " + what)


# ---- column scan -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nbins", [2, 4, 32, 64, 128, 256, 512, 1024])
def test_radix_column_scan(nbins):
    for nrows in (1, 2, 255, 256, 257, 383, 32768, 32769, 40000):      # one workgroup up to 256 rows, two levels, three above 256 x 128
        top = ((1 << 32) - 1) // (nrows * nbins)      # every count <= top: the total stays below 2^32
        rows = _rng(16, nbins, nrows).integers(0, min(top, 1 << 20) + 1, (nrows, nbins), dtype=np.uint64).astype(np.uint32)
        _eq(pu.column_scan(rows), pu.column_scan_ref(rows), "radix_column_scan nbins=%d nrows=%d" % (nbins, nrows))


# ---- CSR sort ----------------------------------------------------------------------------------------------------------------------------
def _bits_of(M):
    return max(1, (M - 1).bit_length())


def _csr_fin(mb, fmt):
    """Field widths as matrix.hip's CSR build guarantees them: mb + idbits + pb + 2 <= 64 and rs >= idbits + pb + 2; with inline partners
    rs = 63 - mb (bit 63 is the flag), pbi = min(pb, (rs - (mb - 1)) / 2) >= 10, positions below 2^16 (pb <= 16)."""
    idbits, pb = 20, 12
    if fmt == "plain":
        fin = dict(idbits=idbits, pb=pb, rs=idbits + pb + 2, mb=mb, pbi=0)
    else:
        rs = 63 - mb
        fin = dict(idbits=idbits, pb=pb, rs=rs, mb=mb, pbi=min(pb, (rs - (mb - 1)) // 2))
        assert fin["pbi"] >= 10 and mb >= 2
    assert mb + idbits + pb + 2 <= 64 and fin["rs"] >= idbits + pb + 2 and fin["rs"] + mb <= 64
    return fin


def _csr_words(rows_with_counts, M, fin, fmt, seed):
    """Keys in CSC order — k-mer id ascending, the reads of one id together — for rows given as {read: number of entries}"""
    rng = _rng(17, seed, M)
    reads = np.repeat(np.array(list(rows_with_counts.keys()), dtype=np.int64), list(rows_with_counts.values()))
    n = reads.size
    kid = np.sort(rng.integers(0, 1 << fin["idbits"], n))
    reads = reads[rng.permutation(n)]      # which read an entry of a column belongs to
    # (several reads per id: ids repeat about n / 2^20 times by chance; make columns on purpose)
    kid = (kid // 3) * 3
    order = np.lexsort((reads, kid))       # inside a column the reads ascend, as the k-mer stage writes them
    kid, reads = kid[order], reads[order]
    hint, pos = rng.integers(0, 4, n), rng.integers(0, 1 << fin["pb"], n)
    u = U64
    plain = (reads.astype(u) << u(fin["rs"])) | (kid.astype(u) << u(fin["pb"] + 2)) | (hint.astype(u) << u(fin["pb"])) | pos.astype(u)
    if fmt == "plain":
        return plain
    partner, pq, pt = rng.integers(0, M, n), rng.integers(0, 1 << fin["pbi"], n), rng.integers(0, 1 << fin["pbi"], n)
    inl = (u(1) << u(63)) | (reads.astype(u) << u(fin["rs"])) | ((partner.astype(u) >> u(1)) << u(2 * fin["pbi"])) | (pq.astype(u) << u(fin["pbi"])) | pt.astype(u)
    if fmt == "inline":
        return inl
    return np.where(rng.integers(0, 2, n) == 1, inl, plain)


def _check_csr(rows, M, mb, fmt, seed, what):
    fin = _csr_fin(mb, fmt)
    assert all(0 <= r < M for r in rows) and M <= 1 << mb
    words = _csr_words(rows, M, fin, fmt, seed)
    csr, rowptr = pu.sort_keys_to_csr(words, fin, M)
    wcsr, wrowptr = pu.csr_unpack_ref(words, fin, M)
    _eq(rowptr, wrowptr, what + " rowptr")
    _eq(csr, wcsr, what + " csr")
    assert int(rowptr[0]) == 0 and int(rowptr[M]) == words.size and (np.diff(rowptr.astype(np.int64)) >= 0).all()


def _formats(mb):
    return ("plain",) if mb < 2 else ("plain", "inline", "mixed")


@pytest.mark.parametrize("mb", [1, 9, 10, 18, 19])
def test_csr_sort_digit_splits_and_empty_rows(mb):
    """one to three passes; empty rows at the start, at the end and in runs of thousands; a read whose entries span three tiles; rows behind
    the last entry"""
    rng = _rng(18, mb)
    for M in sorted({1 << mb, max(1, (1 << mb) - 3), max(1, (1 << mb) // 2 + 1)} | ({1} if mb == 1 else set())):
        for fmt in _formats(mb):
            # every row a few entries
            if M <= 4096:
                _check_csr({r: int(rng.integers(1, 6)) for r in range(M)}, M, mb, fmt, 1, "mb=%d M=%d %s dense" % (mb, M, fmt))
            # sparse: rows 0 .. first empty, runs of thousands empty (large M), the last rows empty; one read of 2 tiles + 3 entries (spans three tiles)
            first = min(M - 1, 5)
            rows = {first: 2 * TILE + 3}
            for r in rng.integers(first, max(first + 1, M - M // 8 - 1), 40):
                rows[int(r)] = rows.get(int(r), 0) + int(rng.integers(1, 4))
            _check_csr(rows, M, mb, fmt, 2, "mb=%d M=%d %s sparse" % (mb, M, fmt))
            # a few entries only, in the first and the last row
            _check_csr({0: 1, M - 1: 2} if M > 1 else {0: 3}, M, mb, fmt, 3, "mb=%d M=%d %s ends" % (mb, M, fmt))


@pytest.mark.parametrize("M", [1, 1023, 1024, 1025, 1024 ** 2 - 1, 1024 ** 2, 1024 ** 2 + 1, 3 * 1024 ** 2 + 5])
def test_csr_sort_row_pointers_across_blocks_and_chunks_of_blocks(M):
    """entries in a few, far-apart rows: the rows between them are closed by the suffix minimum over blocks of 1024 rows, whose carry across
    chunks of 1024 blocks only runs with more than 1024 x 1024 rows"""
    mb = _bits_of(M)
    cand = [0, 1, 1022, 1023, 1024, 1025, 2047, 1024 ** 2 - 1025, 1024 ** 2 - 1024, 1024 ** 2 - 2, 1024 ** 2 - 1, 1024 ** 2, 1024 ** 2 + 1,
            1024 ** 2 + 5, 2 * 1024 ** 2 - 1, 2 * 1024 ** 2 + 4, 3 * 1024 ** 2 - 7, M - 2, M - 1]
    cand = sorted({r for r in cand if 0 <= r < M})
    for fmt in _formats(mb):
        # (a) all of them; (b) only the first quarter of them: every chunk of blocks behind is empty and takes n from rowptr[M];
        # (c) only one row in the last chunk: every row before it takes ITS pointer across the chunk boundaries; (d) one row in the first block
        for tag, rows in (("all", cand), ("front", cand[:max(1, len(cand) // 4)]), ("last", cand[-1:]), ("first", cand[:1]), ("every other", cand[::2])):
            d = {r: 1 + (i % 3) for i, r in enumerate(rows)}
            d[rows[len(rows) // 2]] = 2 * TILE + 3
            _check_csr(d, M, mb, fmt, 4, "M=%d mb=%d %s rows %s" % (M, mb, fmt, tag))


# ---- group offsets -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", ["u64 shift 0", "u64 shift 20", "k32"])
def test_group_offsets(variant):
    k32, shift = variant == "k32", 20 if variant == "u64 shift 20" else 0
    rng = _rng(19, shift, int(k32))

    def check(groups, nkeys, what):
        g = np.asarray(groups, dtype=np.uint64)
        keys = (g << U64(shift)) | (rng.integers(0, 1 << shift, g.size, dtype=np.uint64) if shift else U64(0))      # bits below the shift ride along
        _eq(pu.group_offsets(keys, nkeys, shift, k32=k32), pu.group_offsets_ref(keys, nkeys, shift), "group_offsets %s %s" % (variant, what))

    for nkeys in (0, 1, 1000):
        check([], nkeys, "n=0 nkeys=%d" % nkeys)      # every pointer 0
        assert (pu.group_offsets(np.zeros(0, dtype=np.uint64), nkeys, shift, k32=k32) == 0).all()
    check([0], 1, "one key"); check([7], 8, "one key behind empty groups"); check([7], 100000, "one key, nkeys far behind it")
    check([3] * 1000, 4, "all keys equal"); check([0] * 257, 300000, "all keys in group 0, 3 * 10^5 empty groups behind")
    for n in (255, 256, 257, 511, 512, 513):
        check(np.sort(rng.integers(0, 50, n)), 50, "n=%d dense" % n)
        check(np.sort(rng.integers(0, 20, n)) * 100000, 20 * 100000 + 12345, "n=%d gaps of 10^5 empty groups" % n)
        check(np.arange(n), n, "n=%d one key per group" % n)
    check(np.sort(rng.integers(0, 1 << 11, 100000)), 1 << 11, "10^5 keys")


# ---- fill / reduce_max -------------------------------------------------------------------------------------------------------------------
GRID_N = (0, 1, 255, 256, 257, 4096 * 256 + 1, 2048 * 256 + 1, 3 * 4096 * 256 + 77)      # (the grids cap at 4096 / 2048 workgroups: beyond, a thread takes several places)


def test_fills():
    for n in GRID_N:
        for dtype, v, preset in ((np.uint32, 0xCAFEF00D, 0x11111111), (np.uint64, (1 << 64) - 1, 0x2222222222222222), (np.uint64, 0, 0x2222222222222222)):
            got = pu.fill(dtype, n + 300, v, n, preset)
            want = np.full(n + 300, preset, dtype=dtype)
            want[:n] = v
            _eq(got, want, "fill %s n=%d" % (np.dtype(dtype).name, n))


def test_reduce_max():
    assert pu.reduce_max(np.zeros(0, dtype=np.uint64)) == 0
    for n in GRID_N[1:]:
        base = _rng(20, n).integers(0, 1 << 63, n, dtype=np.uint64)
        for place in sorted({0, n // 2, n - 1}):
            for top in ((1 << 64) - 1, (1 << 63) + 5):
                x = base.copy()
                x[place] = top
                assert pu.reduce_max(x) == top, (n, place, top)
        assert pu.reduce_max(base) == int(base.max())
        assert pu.reduce_max(np.zeros(n, dtype=np.uint64)) == 0
