"""The C++ host mirror of cutting bridges (CutBridges in elba_amd/hostcpp/elba_host.hpp) against the Python binding on one workload: the
same stats, the same cut S and bridge reads (checksums), the same contigs' counts, and the host's own comparison of the cut S with the
uncut one."""
import json
import os
import subprocess

import numpy as np
import pytest

import contig_util as cu
import elba_amd
import util

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "elba_amd", "hostcpp", "test_host_bridges")
FA = os.path.join(util.GOLDEN, "small_err.fa")
# The workload: synth_reads(89, 60000, 12, 3000, 500, error_rate=0.03, min_len=400), k = 17, 2 .. 12, cut at (2, 3).  Its string graph has 218
# entries, 8 anchors, 8 chains and 8 long flanks, and no bridge: a scan on the device of seeds 80 .. 99 x error rate {0.03, 0.08} x
# {no repeats, 4 repeat families of 400 bases on a tenth of the genome} at (1, 3) and (2, 3) found none in any of the 160 graphs (they have
# some 240 reads each), and this is the one with the most chains and long flanks.  So the mirror is held to the binding on a call that
# looks at chains and flanks and removes nothing; tests/test_gpu_bridges.py holds the removal.
SEED, ERR = 89, 0.03
MAX_BRIDGE_READS, MIN_FLANK_READS = 2, 3


def _build():
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "elba_amd", "hostcpp")], stdout=subprocess.DEVNULL)


def _args():
    m = util.golden_meta()["small_err"][0]
    return [BIN, FA, str(m["k"]), str(m["lower"]), str(m["upper"]), str(MAX_BRIDGE_READS), str(MIN_FLANK_READS)]


def test_bridges_mirror_builds_and_fails_loudly_without_gpu():
    _build()
    p = subprocess.run(_args(), capture_output=True, text=True)
    if p.returncode == 3:
        assert "no HIP device" in p.stderr
    else:
        assert p.returncode == 0 and json.loads(p.stdout)["reads"] == 80


@pytest.mark.gpu
def test_bridges_mirror_equals_the_python_binding(tmp_path):
    if not os.path.exists(BIN):
        _build()
    packed, off, lens, _ = elba_amd.synth_reads(SEED, 60000, 12, 3000, 500, error_rate=ERR, min_len=400)
    fa = tmp_path / "reads.fa"
    with open(fa, "w") as f:
        for i, s in enumerate(cu.seqs_of(packed, off, lens)):
            f.write(">r%d\n%s\n" % (i, s))
    got = json.loads(subprocess.run([BIN, str(fa), "17", "2", "12", str(MAX_BRIDGE_READS), str(MIN_FLANK_READS)], capture_output=True, text=True, check=True).stdout)
    e = elba_amd.Engine(17, 2, 12)
    e.set_reads(packed, off, lens)
    e.count_kmers(); e.create_kmer_matrix(); e.create_seed_matrix()
    e.align_seeds()
    e.transitive_reduction(0.65, 1000)
    st = e.cut_bridges(MAX_BRIDGE_READS, MIN_FLANK_READS)
    g = e.export_string_graph()
    cut = np.flatnonzero(e.export_read_flags(len(lens)) & 16)
    cs = e.generate_contigs()
    s_checksum = int(((g["rows"] + 1) * 1000003 + g["cols"] * 10007 + g["vals"]["suffix"].astype(np.int64).astype(np.uint32).astype(np.int64)).sum())
    want = {k: st[k] for k in ("nnz_before", "nnz_after", "anchors", "chains", "long_flanks", "bridges", "reads_removed", "entries_removed")}
    want.update(reads=len(lens), s_checksum=s_checksum, read_checksum=int(((cut + 1) * 10007).sum()), host_equal=1, contigs=cs["contigs"], bases=cs["bases"],
                branches=cs["branches"])
    print("host mirror workload:", want)
    assert got == want
    assert len(cut) == st["reads_removed"] and st["anchors"] > 0 and st["chains"] > 0 and st["long_flanks"] > 0
    e.close()
