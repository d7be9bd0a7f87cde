"""-m gpu: raw FASTA / FASTQ text -> reads on the context with the index built on the device (elba_set_reads_text, text_index.hip).
The device's records and name extents are compared field for field with the restatement of the grammar (tests/text_index_util.py), the
packed bytes, offsets and lengths with the oracle's encoder (po.pack_reads) — at the edges of the passes' tiles and of the scans' spans
(both read from the library), on the FASTA encoder's grid, on FASTQ, at a file offset beyond 2^40, and through every rejection."""
import gzip
import os

import numpy as np
import pytest

import elba_amd
from elba_amd import fasta
import gpu_util as gu
import prim_util as pu
import text_index_util as tx
import trim_util as tu
import util
from oracle import pyoracle as po

pytestmark = pytest.mark.gpu
G = util.GOLDEN


@pytest.fixture(scope="module")
def eng():
    e = elba_amd.Engine(17, 2, 8)
    yield e
    e.close()


@pytest.fixture(scope="module")
def T(eng):
    t = eng.get_stat("text_tile_bytes")
    assert t >= 64 and t % 16 == 0
    return t


_exported, _same_export, _check, _rejected = tx.device_exported, tx.same_export, tx.device_check, tx.device_rejected      # (shared with test_gpu_second_trips.py)


# ---- small shapes and the hand cases -----------------------------------------------------------------------------------------------------
def test_hand_cases_field_for_field(eng):
    for label, data, fmt, recs, names in tx.GOOD_CASES:
        st, _ = _check(eng, data, fmt, loop=True)
        got_names, got = eng.export_read_index()
        assert [(int(r["len"]), int(r["pos"]), int(r["bases"])) for r in got] == recs and got_names == names, label
    st = eng.set_reads_text(b"")
    assert st["nreads"] == 0 and st["format"] == 1 and st["lines"] == 0 and st["packed_bytes"] == 0


def test_each_rejection_alone_leaves_the_old_reads_and_index_and_the_context_usable(eng):
    good = tx.fasta_bytes(tx.random_seqs(np.random.default_rng(1), [70, 0, 5, 130]), 60)
    st, _ = _check(eng, good, file_off=77)
    before = _exported(eng, st["nreads"], st["packed_bytes"])
    for label, data, fmt, kind, off in tx.BAD_CASES:
        (k, o), rec = _rejected(eng, data, fmt)
        assert (k, o) == (kind, off), label
        assert _same_export(_exported(eng, st["nreads"], st["packed_bytes"]), before), label
    assert _rejected(eng, b">a\nAC\n\nAC\n>b\nA\n")[1] == 0 and _rejected(eng, b">a\nAC\n>b\nA\nAC\n")[1] == 1      # the record the message names
    assert _rejected(eng, b"@a\nA\n+\nI\n@b\nAC\n+\nI\n")[1] == 1
    names, _ = eng.export_read_index()
    assert names == ["read0", "read1", "read2", "read3"]
    _check(eng, b">x\nACGT\n")      # the next good call succeeds on the same context


def test_two_errors_in_different_tiles_name_the_earlier_one(eng, T):
    seq = b"ACGT" * (T // 2)
    data = bytearray(b">a\n" + seq[:100] + b"\n" + seq[:50] + b"\n" + seq[:100] + b"\n" + b">b\n" + seq + b"\n" + seq + b"\n>c\nAC\r\n")
    assert len(data) > 4 * T
    assert _rejected(eng, data)[0] == (tx.SHAPE, 104)            # the short middle line of the first tile, not the '\r' of the last
    data[1] = 0x0D
    assert _rejected(eng, data)[0] == (tx.CR, 1)
    data[1] = ord("a"); data[104 + 50:104 + 50] = seq[:50]      # mend the first: the '\r' is what is left
    assert _rejected(eng, data)[0] == (tx.CR, len(data) - 2)
    fq = bytearray(tx.fastq_bytes([seq, seq, seq]))
    fq[-2:-1] = b""                                              # the last quality line one byte short ...
    third = fq.rindex(b"@read2")
    assert _rejected(eng, fq)[0] == (tx.FQ_QUAL, third)
    plus = fq.index(b"\n+\n") + 1
    fq[plus] = ord("-")                                          # ... and the first record's '+' missing, three tiles earlier
    assert _rejected(eng, fq)[0] == (tx.FQ_PLUS, plus)


# ---- the FASTA encoder's grid and the goldens ----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def eng_fai():
    e = elba_amd.Engine(17, 2, 8)
    yield e
    e.close()


def _same_as_set_reads_fasta(e, path, got):
    """the file through the host's index (write_fai) and elba_set_reads_fasta on a context of its own: the same reads"""
    fasta.write_fai(path)
    _, recs = fasta.read_fai(path + ".fai")
    chunk, start = fasta.load_chunk(path, recs)
    st = e.set_reads_fasta(chunk, start, recs)
    assert _same_export(e.export_reads(len(recs), st["packed_bytes"]), got)
    return recs


@pytest.mark.parametrize("width", pu.INGEST_WIDTHS)
def test_fasta_grid_equals_restatement_oracle_and_set_reads_fasta(eng, eng_fai, tmp_path, width):
    seqs = pu.ingest_grid_seqs(width + 1)
    p = str(tmp_path / "grid.fa")
    files = [(seqs, dict(final_newline=True)), (seqs, dict(final_newline=False)), (seqs[::-1], dict(final_newline=True)), (seqs[::-1], dict(final_newline=False))]
    files += [(seqs, dict(place=(i, m))) for i, m in ((1, 5), (7, 11), (1, 15))]
    for order, kw in files:
        pu.write_fasta(p, order, width, **kw)
        data = open(p, "rb").read()
        st, got_seqs = _check(eng, data)
        assert got_seqs == list(order)
        recs = _same_as_set_reads_fasta(eng_fai, p, eng.export_reads(st["nreads"], st["packed_bytes"]))
        assert (eng.export_read_index()[1] == recs).all()
        if "place" in kw:
            assert int(recs[kw["place"][0]]["pos"]) % 16 == kw["place"][1]


def test_pipeline_from_text_equals_the_oracle(eng):
    data = open(os.path.join(G, "small_err.fa"), "rb").read()
    seqs = util.read_fasta(os.path.join(G, "small_err.fa"))
    e = elba_amd.Engine(17, 2, 8)
    st, got = _check(e, data)
    assert got == seqs
    e.count_kmers(); e.create_kmer_matrix(); ost = e.create_seed_matrix()
    packed, off, lens = po.pack_reads(seqs)
    o = gu.oracle_run(packed, off, lens, 17, 2, 8)
    gu.assert_B_equal(e.export_csr(), o.B())
    gu.assert_stats_equal(ost, o)
    e.close()


def test_gzipped_reference_reads_through_set_reads_file(eng):
    p = os.path.join(G, "reads_ref.fa.gz")
    seqs = util.read_fasta(p)
    st = eng.set_reads_file(p)
    wp, woff, wlen = po.pack_reads(seqs)
    got, goff, glen = eng.export_reads(len(seqs), st["packed_bytes"])
    assert st["nreads"] == len(seqs) and (goff == woff).all() and (glen == wlen).all() and (got[:st["packed_bytes"]] == wp[:st["packed_bytes"]]).all()
    names, recs = eng.export_read_index()
    with gzip.open(p, "rb") as f:
        data = f.read()
    want = tx.index_numpy(data)
    assert names == tx.names_of(data, want) and (recs == want["recs"]).all()


@pytest.mark.parametrize("fmt", ["fasta", "fastq"])
def test_reference_compress_vectors(eng, fmt):
    vec = [line.split() for line in open(os.path.join(G, "encode_vectors.txt")) if line[0] != "#"]
    seqs = [v[0].encode() for v in vec]
    data = tx.fasta_bytes(seqs) if fmt == "fasta" else tx.fastq_bytes(seqs)
    st, _ = _check(eng, data)
    got, off, ln = eng.export_reads(len(seqs), st["packed_bytes"])
    for i, v in enumerate(vec):
        assert got[int(off[i]):int(off[i]) + (len(v[0]) + 3) // 4].tobytes().hex() == v[1], v


# ---- tile edges -----------------------------------------------------------------------------------------------------------------------------
def test_tile_edges_fasta(eng, T):
    rng = np.random.default_rng(2)
    s = tx.random_seqs(rng, [4 * T])[0]
    for size in (T - 1, T, T + 1, 2 * T):                                   # a chunk of exactly that many bytes, with and without its final newline
        data = b">r\n" + s[:size - 4] + b"\n"
        assert len(data) == size
        _check(eng, data); _check(eng, data[:-1] + b"A")
    _check(eng, b">r\n" + s[:T - 4] + b"\n>second\nACGT\n")               # '\n' the last byte of a tile, '>' the first of the next
    _check(eng, b">r\n" + s[:T - 3] + b"\n>second\nACGT\n")               # '\n' the first byte of a tile
    _check(eng, b">r\n" + s[:T - 4] + b"\n>")                             # a lone '>' as a tile's only byte
    head = b">r\n" + s[:T - 24] + b"\n"                                    # the next header starts 20 bytes in front of the edge
    assert len(head) == T - 20
    _check(eng, head + b">a_name_across_the_edge_of_the_tile desc\nACGT\n")
    st, _ = _check(eng, head + b">name_ends_on_edge__ desc\nACGT\n")      # the name's last byte is the tile's last
    npos, nlen = eng.export_read_index_raw()[1:]
    assert int(npos[1]) + int(nlen[1]) == T
    _check(eng, head + b">line_ends_on_edge__\nACGT\n")
    _check(eng, b">long\n" + s[:3 * T + 100] + b"\n>b\nAC\n")              # one line longer than three tiles: tiles without a newline
    _check(eng, b">" + s[:3 * T + 100].replace(b" ", b"A") + b" d\nAC\n")  # ... as a header, its name longer than three tiles
    for k in range(1, 18):                                                  # chunk lengths 1 .. 17 modulo 16
        data = b">r\n" + s[:60 + k] + b"\n"
        assert len(data) % 16 == k % 16
        _check(eng, data, loop=True)
        _check(eng, tx.fasta_bytes([s[:T + k], s[:k]], 61), loop=(k == 7))


def test_tile_edges_fastq(eng, T):
    s = tx.random_seqs(np.random.default_rng(3), [2 * T])[0]
    one = lambda L: b"@r\n" + s[:L] + b"\n+\n" + b"I" * L + b"\n"
    for size in (T - 1, T, T + 1, 2 * T):
        L = (size - 7) // 2
        data = one(L) if (size - 7) % 2 == 0 else b"@rr\n" + one(L)[3:]
        assert len(data) == size
        _check(eng, data); _check(eng, data[:-1])
    first = one((T - 7) // 2 if T % 2 else (T - 8) // 2)
    first = first if len(first) == T else b"@rr\n" + first[3:]
    assert len(first) == T
    _check(eng, first + one(5))                                             # '@' the first byte of a tile, '\n' the last of the one before
    _check(eng, first[:3] + b"x" + first[3:] + one(5))                      # '\n' the first byte of a tile
    data = one(T - 13) + b"@b\n" + s[:9] + b"\n+\n" + b"@" * 9 + b"\n"     # a quality line of '@' across an edge
    assert data.index(b"@@@@") == 2 * T - 4
    _check(eng, data)
    for k in range(1, 18):
        _check(eng, one(30 + k)[:-1] if k % 2 else one(30 + k), loop=True)


# ---- scan edges ------------------------------------------------------------------------------------------------------------------------------
def test_more_lines_than_one_scan_span(eng):
    span = eng.get_stat("text_scan_span")
    rng = np.random.default_rng(4)
    seqs = tx.random_seqs(rng, rng.integers(0, 12, span + 5))
    st, _ = _check(eng, tx.fasta_bytes(seqs))                               # 2 (span + 5) lines, span + 5 records: the flag scan and the offset scan recurse
    assert st["lines"] > span and st["nreads"] > span
    st, _ = _check(eng, tx.fastq_bytes(seqs))
    assert st["lines"] > 4 * span
    st, _ = _check(eng, tx.fasta_bytes(tx.random_seqs(rng, [2 * span + 3, 5, span]), 1, final_newline=False))      # one-base lines: the most lines per byte
    assert st["lines"] > 3 * span


def test_more_tiles_than_one_scan_span(eng, T):
    span = eng.get_stat("text_scan_span")
    rng = np.random.default_rng(5)
    nreads = 24
    per = (span + 3) * T // nreads
    seqs = tx.random_seqs(rng, [per + i for i in range(nreads)], alphabet=b"ACGTacgt")
    data = tx.fasta_bytes(seqs, 0)
    assert len(data) > (span + 2) * T
    st, got = _check(eng, data)
    assert got == seqs


@pytest.mark.parametrize("fmt", ["fasta", "fastq"])
def test_more_reads_than_workgroups(eng, fmt):
    rng = np.random.default_rng(77)
    lens = rng.integers(0, 41, 10000)
    lens[:8] = (0, 1, 0, 0, 5, 40, 0, 3)
    seqs = tx.random_seqs(rng, lens)
    st, _ = _check(eng, tx.fasta_bytes(seqs, 7) if fmt == "fasta" else tx.fastq_bytes(seqs))
    assert st["nreads"] == 10000


# ---- FASTQ ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("final", [True, False])
def test_fastq_reads_of_every_encoder_trip_length(eng, final):
    rng = np.random.default_rng(6)
    lengths = [0] + list(pu.INGEST_LENGTHS[:-1]) + ([0] if final else [9])      # an empty read with an empty quality first and (with a final newline) last
    seqs = tx.random_seqs(rng, lengths)
    quals = [bytes(rng.integers(33, 127, len(s)).astype(np.uint8)) for s in seqs]
    for i, lead in ((2, b"@"), (3, b"+"), (4, b">"), (9, b"@")):              # quality lines that begin like a header, a separator, a FASTA header
        quals[i] = lead + quals[i][1:]
    data = tx.fastq_bytes(seqs, quals=quals, final_newline=final)
    st, got = _check(eng, data)
    assert got == seqs and max(lengths) == 70001
    fq = eng.export_reads(len(seqs), st["packed_bytes"])
    st2, got2 = _check(eng, tx.fasta_bytes(seqs, 80))
    assert got2 == seqs and _same_export(eng.export_reads(len(seqs), st2["packed_bytes"]), fq)      # the same reads as FASTA: identical packed bytes


# ---- offsets ---------------------------------------------------------------------------------------------------------------------------------
def test_file_offset_beyond_2_40_and_first_global_id(eng):
    seqs = util.read_fasta(os.path.join(G, "small_err.fa"))
    data = tx.fasta_bytes(seqs, 60)
    st0, _ = _check(eng, data)
    base = eng.export_read_index_raw(), eng.export_reads(st0["nreads"], st0["packed_bytes"])
    off = (1 << 40) + 5
    st, _ = _check(eng, data, file_off=off)
    recs, npos, nlen = eng.export_read_index_raw()
    assert (recs["pos"] - base[0][0]["pos"] == off).all() and (npos - base[0][1] == off).all() and (recs["len"] == base[0][0]["len"]).all()
    assert _same_export(eng.export_reads(st["nreads"], st["packed_bytes"]), base[1])
    assert _rejected(eng, b">a\nAC\n\nAC\n", file_off=off)[0] == (tx.SHAPE, off + 6)
    # first_global_id: the rows of the k-mer matrix carry it, as after elba_set_reads
    mats = []
    for gid, text in ((0, True), (1000, True), (1000, False)):
        e = elba_amd.Engine(17, 2, 8)
        if text:
            e.set_reads_text(data, 0, "auto", gid)
        else:
            e.set_reads(*po.pack_reads(seqs), first_global_id=gid)
        e.count_kmers(); e.create_kmer_matrix()
        mats.append(e.export_kmer_matrix())
        e.close()
    assert mats[0]["Z"] > 0 and (mats[1]["csc_read"] - mats[0]["csc_read"] == 1000).all()
    assert (mats[1]["csc_read"] == mats[2]["csc_read"]).all() and (mats[1]["csc_pos"] == mats[2]["csc_pos"]).all()


# ---- state -----------------------------------------------------------------------------------------------------------------------------------
def _status(f, *a):
    with pytest.raises(elba_amd.ElbaError) as x:
        f(*a)
    return x.value.status


def test_the_index_belongs_to_the_read_set():
    e = elba_amd.Engine(17, 2, 8)
    assert _status(e.export_read_index) == 5                                # before any text call
    seqs = tx.random_seqs(np.random.default_rng(8), [100, 120, 90, 100], alphabet=b"ACGT")
    packed, off, lens = po.pack_reads(seqs)
    e.set_reads(packed, off, lens)
    assert _status(e.export_read_index) == 5
    _check(e, tx.fasta_bytes(seqs, 60))
    e.set_reads(packed, off, lens)                                          # replaced by elba_set_reads
    assert _status(e.export_read_index) == 5 and _status(e.export_read_index_raw) == 5
    _check(e, tx.fastq_bytes(seqs))
    chunk = tx.fasta_bytes(seqs, 60)
    want = tx.index_numpy(chunk)
    e.set_reads_fasta(chunk, 0, want["recs"])                               # replaced by elba_set_reads_fasta
    assert _status(e.export_read_index) == 5
    _check(e, tx.fasta_bytes(seqs, 60))
    rows, cols, vals = tu.overlaps_for(4, [(0, 10, 80), (1, 0, 60)])
    e.set_overlaps(4, rows, cols, vals)
    e.read_pileup(mode=1, margin=0, min_depth=1, min_run=1, trim_len=0)
    e.trim_reads(mode=1, min_len=1)
    assert e.export_read_index()[0] == ["read0", "read1", "read2", "read3"]      # pileup and trim leave the reads, and so the index
    e.adopt_trimmed_reads()                                                 # replaced by the trimmed pieces
    assert _status(e.export_read_index) == 5
    _check(e, b">again\nACGT\n")
    e.close()


def test_one_context_over_a_large_an_empty_a_small_and_a_fastq_chunk(T):
    e = elba_amd.Engine(17, 2, 8)
    rng = np.random.default_rng(9)
    big = tx.random_seqs(rng, rng.integers(0, 3000, 400))
    _check(e, tx.fasta_bytes(big, 70))
    st, _ = _check(e, b"")
    assert st["nreads"] == 0 and e.export_read_index()[0] == []
    _check(e, b">s\nACGTN\n", loop=True)
    _check(e, tx.fastq_bytes(big[:50]))
    _check(e, b"", "fastq")
    _check(e, tx.fasta_bytes(big, 70))
    e.close()
