"""The C++ host mirror of the trim stage (TrimReads, ExportTrimMap, TrimmedReadsDevice, AdoptTrimmedReads in elba_amd/hostcpp/elba_host.hpp)
against the Python binding on one workload: the same map and packed bytes (checksums), every base of every piece equal to its source's on
the host, and the same k-mer instances counted on the adopted pieces."""
import os

import numpy as np
import pytest

import elba_amd
import hostcpp_util as hu
import util
from oracle import pyoracle as po

FA = os.path.join(util.GOLDEN, "small_err.fa")
CFG = dict(mode=1, margin=20, min_depth=2, min_run=300, trim_len=500)
TRIM = dict(mode=1, min_len=50)


def _args():
    m = util.golden_meta()["small_err"][0]
    return ([hu.binary("test_host_trim"), FA, str(m["k"]), str(m["lower"]), str(m["upper"])] + [str(CFG[k]) for k in ("mode", "margin", "min_depth", "min_run", "trim_len")] +
            [str(TRIM["mode"]), str(TRIM["min_len"])])


def test_trim_mirror_builds_and_fails_loudly_without_gpu():
    got = hu.runs_or_reports_no_device(_args())
    assert got is None or got["reads"] == 80


@pytest.mark.gpu
def test_trim_mirror_equals_the_python_binding():
    args = _args()
    got = hu.run_json(args[0], args[1:])
    m = util.golden_meta()["small_err"][0]
    packed, off, lens = po.pack_reads(util.read_fasta(FA))
    e = elba_amd.Engine(m["k"], m["lower"], m["upper"])
    e.set_reads(packed, off, lens)
    e.count_kmers(); e.create_kmer_matrix(); e.create_seed_matrix()
    e.align_seeds()
    e.read_pileup(**CFG)
    st = e.trim_reads(**TRIM)
    mp = e.export_trim_map()
    e.adopt_trimmed_reads()
    pk, _, _ = e.export_reads(st["pieces"], st["packed_bytes"])
    ks = e.count_kmers()
    map_checksum = int(((mp["src_read"] + 1) * 1000003 + mp["src_beg"].astype(np.int64) * 10007 + mp["src_end"]).sum())
    w = (np.arange(st["packed_bytes"], dtype=np.int64) % 1000003) + 1
    byte_checksum = int((pk[:st["packed_bytes"]].astype(np.int64) * w).sum())
    want = {"reads": 80, "pieces": st["pieces"], "reads_split": st["reads_split"], "reads_dropped": st["reads_dropped"], "bases_out": st["bases_out"],
            "packed_bytes": st["packed_bytes"], "map_checksum": map_checksum, "byte_checksum": byte_checksum, "host_equal": 1,
            "kmer_reads": ks["nreads"], "kmer_instances": ks["instances"]}
    assert got == want
    assert st["pieces"] > 0 and st["bases_out"] > 0
    e.close()
