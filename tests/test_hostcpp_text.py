"""The C++ host mirror of the text ingest (set_reads_text in elba_amd/hostcpp/elba_host.hpp) against the Python binding on a FASTA and a
FASTQ file: the same reads, bases, lines and format, the same .fai records, names and packed bytes (checksums)."""
import os

import numpy as np
import pytest

import elba_amd
import hostcpp_util as hu
import text_index_util as tx
import util

FA = os.path.join(util.GOLDEN, "small_err.fa")


def test_text_mirror_builds_and_fails_loudly_without_gpu():
    got = hu.runs_or_reports_no_device([hu.binary("test_host_text"), FA])
    assert got is None or got["reads"] == len(util.read_fasta(FA))


def _u64sum(x):
    return int(np.asarray(x, dtype=np.uint64).sum(dtype=np.uint64))


@pytest.mark.gpu
@pytest.mark.parametrize("fmt", ["fasta", "fastq"])
def test_text_mirror_equals_the_python_binding(tmp_path, fmt):
    seqs = util.read_fasta(FA)
    names = [b"r%d/%d extra words" % (i, len(s)) for i, s in enumerate(seqs)]
    path = str(tmp_path / ("reads." + fmt))
    with open(path, "wb") as f:
        f.write(tx.fasta_bytes(seqs, 70, names=names) if fmt == "fasta" else tx.fastq_bytes(seqs, names=names))
    got = hu.run_json(hu.binary("test_host_text"), [path])
    e = elba_amd.Engine(17, 2, 8)
    st = e.set_reads_file(path)
    rnames, recs = e.export_read_index()
    packed, off, ln = e.export_reads(st["nreads"], st["packed_bytes"])
    e.close()
    i1 = np.arange(1, len(recs) + 1, dtype=np.uint64)
    u = np.uint64
    with np.errstate(over="ignore"):
        rec_checksum = _u64sum(i1 * (recs["len"] * u(1000003) + recs["pos"] * u(10007) + recs["bases"]))
        name_checksum = sum((i + 1) * 131 * len(n) + sum((j + 1) * c for j, c in enumerate(n.encode())) for i, n in enumerate(rnames)) % (1 << 64)
        pb = st["packed_bytes"]
        packed_checksum = _u64sum(np.arange(1, pb + 1, dtype=np.uint64) * packed[:pb].astype(np.uint64))
    want = dict(reads=len(seqs), bases=int(ln.sum()), stat_bases=st["bases"], lines=st["lines"], format=st["format"], packed_bytes=pb, rec_checksum=rec_checksum,
                name_checksum=name_checksum, packed_checksum=packed_checksum)
    print("host mirror workload:", want)
    assert got == want
    assert rnames == ["r%d/%d" % (i, len(s)) for i, s in enumerate(seqs)] and st["format"] == (1 if fmt == "fasta" else 2)
