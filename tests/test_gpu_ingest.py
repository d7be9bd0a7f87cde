"""-m gpu: FASTA chunk -> 2-bit DnaBuffer on the device (elba_set_reads_fasta) against the oracle's encoder and the reference's own
DnaSeq::compress vectors (tests/golden/encode_vectors.txt); reads of several trips of the encode kernel on wrapped lines, empty records, more
reads than workgroups, chunks at unaligned file offsets, and the argument checks."""
import os

import numpy as np
import pytest

import elba_amd
from elba_amd import fasta
import gpu_util as gu
import prim_util as pu
import util
from oracle import pyoracle as po

pytestmark = pytest.mark.gpu
G = util.GOLDEN


def _write_fasta(path, seqs, width, **kw):
    """one record per read, lines of `width` bases (<= 0: one line); an empty read is a header and an empty line (prim_util.write_fasta)"""
    pu.write_fasta(path, seqs, width, **kw)


def _ingest_and_compare(path, seqs, lo=0, hi=None):
    fasta.write_fai(path)
    names, recs = fasta.read_fai(path + ".fai")
    assert len(recs) == len(seqs) and [int(r["len"]) for r in recs] == [len(s) for s in seqs]
    hi = len(seqs) if hi is None else hi
    chunk, start = fasta.load_chunk(path, recs[lo:hi])
    e = elba_amd.Engine(17, 2, 8)
    st = e.set_reads_fasta(chunk, start, recs[lo:hi], first_global_id=lo)
    want, woff, wlen = po.pack_reads(seqs[lo:hi])
    assert st["nreads"] == hi - lo and st["bases"] == int(wlen.sum())
    got, goff, glen = e.export_reads(hi - lo, st["packed_bytes"])
    assert (goff == woff).all() and (glen == wlen).all()
    assert (got[:st["packed_bytes"]] == want[:st["packed_bytes"]]).all()
    return e, (want, woff, wlen)


def test_reference_compress_vectors_through_the_gpu_encoder(tmp_path):
    """every ASCII string of the reference-generated encode vectors, as one FASTA record each (lengths 1.., N/n, lower case)"""
    vec = [line.split() for line in open(os.path.join(G, "encode_vectors.txt")) if line[0] != "#"]
    seqs = [v[0].encode() for v in vec]
    p = str(tmp_path / "vec.fa")
    _write_fasta(p, seqs, 0)
    fasta.write_fai(p)
    names, recs = fasta.read_fai(p + ".fai")
    chunk, start = fasta.load_chunk(p, recs)
    e = elba_amd.Engine(17, 2, 8)
    st = e.set_reads_fasta(chunk, start, recs)
    got, off, ln = e.export_reads(len(seqs), st["packed_bytes"])
    for i, v in enumerate(vec):
        nb = (len(v[0]) + 3) // 4
        assert got[int(off[i]):int(off[i]) + nb].tobytes().hex() == v[1], (v[0], v[1])
    e.close()


@pytest.mark.parametrize("width", [0, 60, 61, 7, 1])
def test_wrapped_fasta_any_line_width_and_rank_chunks(tmp_path, width):
    rng = np.random.default_rng(width + 1)
    alphabet = np.frombuffer(b"ACGTacgtNnXR", dtype=np.uint8)       # incl. characters outside the code table (code 4 is ORed in, src/DnaSeq.cpp:18-24)
    seqs = [alphabet[rng.integers(0, len(alphabet) if i % 3 == 0 else 8, int(rng.integers(1, 700)))].tobytes() for i in range(60)]
    p = str(tmp_path / ("w%d.fa" % width))
    _write_fasta(p, seqs, width)
    e, _ = _ingest_and_compare(p, seqs)
    e.close()
    # a rank's share: records [17, 43) from its own chunk of the file (src/FastaIndex.cpp:222-241)
    e, _ = _ingest_and_compare(p, seqs, 17, 43)
    e.close()


def test_pipeline_from_fasta_equals_pipeline_from_packed_reads(tmp_path):
    import shutil
    seqs = util.read_fasta(os.path.join(G, "small_err.fa"))
    p = str(tmp_path / "small_err.fa")
    shutil.copy(os.path.join(G, "small_err.fa"), p)
    e, (packed, off, lens) = _ingest_and_compare(p, seqs)
    ks = e.count_kmers(); e.create_kmer_matrix(); st = e.create_seed_matrix()
    o = gu.oracle_run(packed, off, lens, 17, 2, 8)
    gu.assert_B_equal(e.export_csr(), o.B())
    gu.assert_stats_equal(st, o)
    e.close()


# ---- the encode kernel's trips of 4096 bases, wrapped lines, and the edges of a chunk -------------------------------------------------
@pytest.mark.parametrize("width", pu.INGEST_WIDTHS)
def test_reads_of_several_trips_on_wrapped_lines(tmp_path, width):
    """lengths around one, two and three trips of 4096 bases, a read of 70 001, the shortest reads and an empty record, at this line width:
    the whole file, the same file without its final newline, the same reads in reverse order (the last record a long one that ends the file
    without a newline), and a rank's chunk whose first record starts at a file offset that is 5, 11 and 15 modulo 16"""
    seqs = pu.ingest_grid_seqs(width + 1)
    assert [len(s) for s in seqs] == list(pu.INGEST_LENGTHS)
    p = str(tmp_path / ("trips%d.fa" % width))
    _write_fasta(p, seqs, width)
    e, _ = _ingest_and_compare(p, seqs)
    e.close()
    _write_fasta(p, seqs, width, final_newline=False)
    e, _ = _ingest_and_compare(p, seqs)
    e.close()
    _write_fasta(p, seqs[::-1], width, final_newline=False)
    assert not open(p, "rb").read().endswith(b"\n")
    e, _ = _ingest_and_compare(p, seqs[::-1])
    e.close()
    for mod16 in (5, 11, 15):
        for lo in (1, 7):      # the chunk starts with a read of 4096 / of 70 001 bases
            _write_fasta(p, seqs, width, place=(lo, mod16))
            fasta.write_fai(p)
            _, recs = fasta.read_fai(p + ".fai")
            assert int(recs[lo]["pos"]) % 16 == mod16 and fasta.load_chunk(p, recs[lo:])[1] == int(recs[lo]["pos"])
            e, _ = _ingest_and_compare(p, seqs, lo, len(seqs))
            e.close()


@pytest.mark.parametrize("width", [0, 7])
def test_more_reads_than_workgroups_at_every_alignment(tmp_path, width):
    """10 000 reads of 0 .. 40 bases: more than num_cus * 16 workgroups' worth (the grid-stride loop), packed offsets at every alignment
    modulo 4 (the 32-bit store and the byte-store fall-back), empty records between the others"""
    rng = np.random.default_rng(77 + width)
    alphabet = np.frombuffer(pu.INGEST_ALPHABET, dtype=np.uint8)
    lens = rng.integers(0, 41, 10000)
    lens[:8] = (0, 1, 0, 0, 5, 40, 0, 3)
    seqs = [alphabet[rng.integers(0, len(alphabet) if i % 3 == 0 else 8, int(n))].tobytes() for i, n in enumerate(lens)]
    p = str(tmp_path / ("many%d.fa" % width))
    _write_fasta(p, seqs, width)
    e, (_, woff, _) = _ingest_and_compare(p, seqs)
    assert {int(o) % 4 for o in woff} == {0, 1, 2, 3}
    e.close()
    e, _ = _ingest_and_compare(p, seqs, 4999, 9000)
    e.close()


def test_argument_checks_leave_the_context_usable(tmp_path):
    seqs = pu.ingest_grid_seqs(5, lengths=(100, 61, 4097, 7))
    p = str(tmp_path / "args.fa")
    _write_fasta(p, seqs, 60)
    fasta.write_fai(p)
    _, recs = fasta.read_fai(p + ".fai")
    chunk, start = fasta.load_chunk(p, recs)
    e = elba_amd.Engine(17, 2, 8)
    with pytest.raises(elba_amd.ElbaError, match="before the chunk"):
        e.set_reads_fasta(chunk, start + 1, recs)
    with pytest.raises(elba_amd.ElbaError, match="past the chunk"):
        e.set_reads_fasta(chunk[:-2], start, recs)            # (the chunk ends with the last record's last base and its newline)
    with pytest.raises(elba_amd.ElbaError, match="past the chunk"):
        e.set_reads_fasta(chunk[:int(recs[2]["pos"]) - start + 100], start, recs)      # cut inside the third record
    bad = recs.copy()
    bad["bases"][1] = 0
    with pytest.raises(elba_amd.ElbaError, match="zero line width"):
        e.set_reads_fasta(chunk, start, bad)
    # the same context still encodes
    st = e.set_reads_fasta(chunk, start, recs)
    want, woff, wlen = po.pack_reads(seqs)
    got, goff, glen = e.export_reads(len(seqs), st["packed_bytes"])
    assert (goff == woff).all() and (glen == wlen).all() and (got[:st["packed_bytes"]] == want[:st["packed_bytes"]]).all()
    e.close()
