"""CPU side of the primitive tests: the references of tests/prim_util.py against brute-force loops (a reference nobody checked proves
nothing), radix_digits restated against the library's own radix_sort_where, the harness library itself, and the FASTA encode kernel's index
arithmetic (trips, staged span, line wraps) restated in Python against the oracle's encoder.  Nothing here needs a GPU."""
import os

import numpy as np
import pytest

import prim_util as pu
from elba_amd import fasta
from oracle import pyoracle as po


def _rng(seed):
    return np.random.default_rng(seed)


# ---- references against loops ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lo,hi", [(0, 1), (0, 3), (5, 9), (0, 64), (40, 64), (63, 64), (7, 7), (9, 3)])
def test_stable_order_against_an_insertion_sort(lo, hi):
    rng = _rng(lo * 64 + hi)
    keys = rng.integers(0, 1 << 64, 40, dtype=np.uint64)
    if hi - lo > 3:
        keys[rng.integers(0, 40, 25)] = keys[3]        # ties, so that stability shows
    width = max(hi - lo, 0)
    field = [(int(k) >> lo) & ((1 << width) - 1) for k in keys]
    order = []
    for i in range(len(keys)):                          # insertion behind every element that is not larger: stable by construction
        at = len(order)
        while at > 0 and field[order[at - 1]] > field[i]:
            at -= 1
        order.insert(at, i)
    if hi > lo:
        assert list(pu.stable_order(keys, lo, hi)) == order
        assert [int(x) for x in pu.sort_field(keys, lo, hi)] == field


def test_group_offsets_reference_against_a_loop():
    for shift in (0, 20):
        g = np.sort(_rng(shift).integers(0, 50, 37)).astype(np.uint64)
        keys = (g << np.uint64(shift)) | np.uint64(5 if shift else 0)
        for nkeys in (50, 64, 200):
            want = [next((z for z in range(len(g)) if int(g[z]) >= k), len(g)) for k in range(nkeys + 1)]
            assert list(pu.group_offsets_ref(keys, nkeys, shift)) == want
    assert list(pu.group_offsets_ref(np.zeros(0, dtype=np.uint64), 4)) == [0] * 5


def test_column_scan_reference_against_a_loop():
    rows = _rng(3).integers(0, 9, (7, 4)).astype(np.uint32)
    want = np.zeros_like(rows)
    for t in range(7):
        for d in range(4):
            want[t, d] = sum(int(rows[tt, dd]) for tt in range(7) for dd in range(d)) + sum(int(rows[tt, d]) for tt in range(t))
    assert (pu.column_scan_ref(rows) == want).all()
    # what the places mean: scattering every tile's digits to them is the stable sort by digit
    digits = _rng(4).integers(0, 4, 7 * 5)
    rows = np.array([[int((digits[t * 5:(t + 1) * 5] == d).sum()) for d in range(4)] for t in range(7)], dtype=np.uint32)
    place = pu.column_scan_ref(rows).astype(np.int64)
    out = np.full(35, -1)
    for z, d in enumerate(digits):
        out[place[z // 5, d]] = z
        place[z // 5, d] += 1
    assert list(out) == list(np.argsort(digits, kind="stable"))


def test_exclusive_scan_reference():
    x = _rng(5).integers(0, 1 << 32, 33, dtype=np.uint64).astype(np.uint32)
    want, run = [], 0
    for v in x:
        want.append(run); run += int(v)
    assert [int(v) for v in pu.exclusive_scan_exact(x)] == want
    assert pu.exclusive_scan_exact(np.zeros(0, dtype=np.uint32)).size == 0 and list(pu.exclusive_scan_exact([9])) == [0]


def _csr_loop(words, fin, M):
    rs, mb, pb, pbi, idbits = fin["rs"], fin["mb"], fin["pb"], fin["pbi"], fin["idbits"]
    rows = [[] for _ in range(M)]
    for w in (int(x) for x in words):
        rows[(w >> rs) & ((1 << mb) - 1)].append(w)
    csr, rowptr = [], []
    for r in range(M):
        rowptr.append(len(csr))
        for w in rows[r]:
            if w >> 63:
                pm = (1 << pbi) - 1
                csr.append((1 << 63) | (((w >> (2 * pbi)) & ((1 << (mb - 1)) - 1)) << 32) | ((w >> pbi) & pm) | ((w & pm) << 16))
            else:
                csr.append((((w >> (pb + 2)) & ((1 << idbits) - 1)) << 32) | (((w >> pb) & 3) << 30) | (w & ((1 << pb) - 1)))
    rowptr.append(len(csr))
    return csr, rowptr


def test_csr_reference_against_a_loop_and_its_fields_round_trip():
    rng = _rng(6)
    M, mb = 23, 5
    fin = dict(idbits=20, pb=12, rs=63 - mb, mb=mb, pbi=12)      # rs >= idbits + pb + 2; 2 pbi + (mb - 1) <= rs
    words, fields = [], []
    for kid in range(30):
        for read in sorted(rng.choice([0, 1, 2, 9, 10, 22], 3, replace=False)):
            if rng.integers(0, 2):
                f = (int(read), kid, int(rng.integers(0, 4)), int(rng.integers(0, 1 << 12)))
                words.append(pu.csr_plain_word(*f, fin)); fields.append(("p",) + f)
            else:
                f = (int(read), int(rng.integers(0, M)), int(rng.integers(0, 1 << 12)), int(rng.integers(0, 1 << 12)))
                words.append(pu.csr_inline_word(*f, fin)); fields.append(("i",) + f)
    csr, rowptr = pu.csr_unpack_ref(np.array(words, dtype=np.uint64), fin, M)
    lcsr, lrowptr = _csr_loop(words, fin, M)
    assert [int(x) for x in csr] == lcsr and [int(x) for x in rowptr] == lrowptr
    # every entry carries its fields: the rows in input order
    it = {r: iter([f for f in fields if f[1] == r]) for r in range(M)}
    for r in range(M):
        for z in range(lrowptr[r], lrowptr[r + 1]):
            f, e = next(it[r]), lcsr[z]
            if f[0] == "p":
                assert e >> 63 == 0 and e >> 32 == f[2] and (e >> 30) & 3 == f[3] and e & ((1 << 30) - 1) == f[4]
            else:
                assert e >> 63 == 1 and (e >> 32) & 0x7FFFFFFF == f[2] >> 1 and e & 0xFFFF == f[3] and (e >> 16) & 0xFFFF == f[4]


# ---- radix_digits ------------------------------------------------------------------------------------------------------------------------
def test_radix_digits_cover_the_bits_with_even_digits():
    for lo in range(0, 64):
        for hi in range(lo + 1, 65):
            d = pu.radix_digits(lo, hi)
            assert d[0][0] == lo and d[-1][0] + d[-1][1] == hi and all(a[0] + a[1] == b[0] for a, b in zip(d, d[1:]))
            widths = [b for _, b in d]
            assert 1 <= min(widths) and max(widths) <= pu.RS_MAXBITS and max(widths) - min(widths) <= 1 and widths == sorted(widths, reverse=True)
            assert len(d) == -(-(hi - lo) // pu.RS_MAXBITS)
    assert pu.radix_digits(0, 34) == [(0, 9), (9, 9), (18, 8), (26, 8)]


def test_harness_builds_and_every_entry_point_resolves():
    L = pu.lib()
    assert os.path.exists(pu.PRIMCHECK_LIB)
    for name in pu.ENTRY_POINTS:
        assert getattr(L, name) is not None, name
    assert L.primcheck_last_error().decode() == ""


def test_radix_sort_where_is_the_parity_of_radix_digits():
    for lo in range(0, 64):
        for hi in range(lo + 1, 65):
            assert pu.sort_where(1000, lo, hi) == len(pu.radix_digits(lo, hi)) & 1 == pu.sort_where_ref(1000, lo, hi), (lo, hi)
    for n, lo, hi in ((0, 0, 64), (1, 0, 64), (5, 7, 7), (5, 9, 3)):
        assert pu.sort_where(n, lo, hi) == 0 == pu.sort_where_ref(n, lo, hi)


# ---- write_fai --------------------------------------------------------------------------------------------------------------------------
def test_write_fai_places_every_record_of_the_grid(tmp_path):
    seqs = pu.ingest_grid_seqs(1)
    for width in (7, 4096, 0):
        for final_newline in (True, False):
            p = str(tmp_path / ("g%d_%d.fa" % (width, final_newline)))
            pu.write_fasta(p, seqs, width, final_newline=final_newline)
            data = open(p, "rb").read()
            fasta.write_fai(p)
            names, recs = fasta.read_fai(p + ".fai")
            assert names == ["read%d" % i for i in range(len(seqs))]
            for r, s in zip(recs, seqs):
                assert int(r["len"]) == len(s) and int(r["bases"]) > 0
                got = bytes(data[int(r["pos"]) + b + b // int(r["bases"])] for b in range(0, len(s), max(1, len(s) // 50)))
                assert got == s[::max(1, len(s) // 50)]
            start, end = fasta.chunk_bounds(recs, len(data))
            assert start == int(recs[0]["pos"]) and end <= len(data)


# ---- the encode kernel's index arithmetic (ingest.hip: k_fasta_encode), restated lane by lane ---------------------------------------
ENC_THREADS = 256
ENC_BASES = 16 * ENC_THREADS
ENC_SPAN = 2 * ENC_BASES + 32
_CODE = np.full(256, 4, dtype=np.uint32)
for _c, _v in ((b"AaNn", 0), (b"Cc", 1), (b"Gg", 2), (b"Tt", 3)):
    for _b in _c:
        _CODE[_b] = _v


def encode_emulated(chunk, chunk_off, rec_len, rec_pos, rec_bases):
    """One record through k_fasta_encode's arithmetic: trips of 4096 bases, each staging the file bytes [a0, f1) in a span of ENC_SPAN bytes
    and every lane picking 16 bases at span[sbase + p + line], sbase = (rec0 - a0) mod 2^32.  Returns the packed bytes; raises when an index
    leaves the span (the kernel would read LDS it did not write)."""
    chunk = np.frombuffer(chunk, dtype=np.uint8)
    M32 = 0xFFFFFFFF
    ln = int(rec_len)
    bases = min(int(rec_bases), M32)
    rec0 = int(rec_pos) - int(chunk_off)
    nbytes = (ln + 3) // 4
    nwords = (nbytes + 3) // 4
    out = np.zeros(4 * nwords, dtype=np.uint8)
    for w0 in range(0, nwords, ENC_THREADS):
        pb = 16 * w0
        pe = min(pb + ENC_BASES, ln)
        f0 = rec0 + pb + pb // bases
        f1 = rec0 + (pe - 1) + (pe - 1) // bases + 1
        a0 = f0 & ~15
        nvec = (f1 - a0 + 15) // 16
        assert 16 * nvec <= ENC_SPAN, "the trip's file bytes do not fit the span"
        span = np.full(ENC_SPAN, 0xEE, dtype=np.uint8)      # (never-written LDS: any use of it shows as a wrong code)
        staged = np.full(16 * nvec, 0x58, dtype=np.uint8)   # 'X' beyond the chunk
        have = max(0, min(a0 + 16 * nvec, chunk.size) - a0)
        staged[:have] = chunk[a0:a0 + have]
        span[:16 * nvec] = staged
        w = w0 + np.arange(ENC_THREADS, dtype=np.int64)
        live = w < nwords
        p0 = 16 * w
        line = p0 // bases
        rem = p0 - line * bases
        word = np.zeros(ENC_THREADS, dtype=np.uint32)
        sbase = (rec0 - a0) & M32
        for i in range(16):
            on = live & (p0 + i < ln)
            idx = (sbase + p0 + i + line) & M32
            assert (idx[on] < 16 * nvec).all(), "a lane reads outside the staged bytes"
            code = _CODE[span[np.where(on, idx, 0)]]
            byte = (code << np.uint32(6 - 2 * (i & 3))) & np.uint32(0xFF)
            word |= np.where(on, byte << np.uint32(8 * (i >> 2)), 0).astype(np.uint32)
            rem = np.where(on, rem + 1, rem)
            wrap = on & (rem == bases)
            rem = np.where(wrap, 0, rem)
            line = np.where(wrap, line + 1, line)
        nlive = int(live.sum())
        out[4 * w0:4 * (w0 + nlive)] = word[:nlive].astype("<u4").view(np.uint8)
    return out[:nbytes]


@pytest.mark.parametrize("width", pu.INGEST_WIDTHS)
def test_encode_arithmetic_on_the_length_and_width_grid(tmp_path, width):
    """every length of the grid at this line width, with and without the final newline, the whole file as the chunk and a rank's chunk that
    starts at file offsets 5, 11 and 15 modulo 16: the kernel's arithmetic gives the oracle encoder's bytes"""
    seqs = pu.ingest_grid_seqs(width + 1)
    for final_newline, mod16, lo in ((True, None, 0), (False, None, 0), (True, 5, 1), (True, 11, 1), (True, 15, 1)):
        p = str(tmp_path / "e.fa")
        pu.write_fasta(p, seqs, width, final_newline=final_newline, place=None if mod16 is None else (lo, mod16))
        fasta.write_fai(p)
        _, recs = fasta.read_fai(p + ".fai")
        assert mod16 is None or int(recs[lo]["pos"]) % 16 == mod16
        chunk, start = fasta.load_chunk(p, recs[lo:])
        want, woff, wlen = po.pack_reads(seqs[lo:])
        for r, o, n in zip(recs[lo:], woff, wlen):
            got = encode_emulated(chunk, start, r["len"], r["pos"], r["bases"])
            nb = (int(n) + 3) // 4
            assert got.size == nb and (got == want[int(o):int(o) + nb]).all(), (width, final_newline, mod16, int(n))
