"""The C++ host mirror of resolving stars (ResolveStars in elba_amd/hostcpp/elba_host.hpp) against the Python binding on one workload: the
same stats, the same resolved S and odd arms (checksums), the same contigs' counts, and the host's own comparison of the resolved S with
the unresolved one."""
import json
import os
import subprocess

import numpy as np
import pytest

import contig_util as cu
import elba_amd
import util

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "elba_amd", "hostcpp", "test_host_stars")
FA = os.path.join(util.GOLDEN, "small_err.fa")
# The workload: synth_reads(92, 60000, 12, 3000, 500, error_rate=0.03, min_len=400), k = 17, 2 .. 12, up to 64 rounds: the R of a real
# reduction, transitive pairs and all.  Its string graph has 230 entries and 6 centres, 2 with one pair in R and 4 with two; 2 reads go, in
# one round.  A scan on the device of seeds 80 .. 99 x error rate {0.03, 0.08} x {no repeats, 4 repeat families of 400 bases on a tenth of
# the genome} found centres in 26 of the 80 graphs (none at 0.08, whose graphs are nearly empty), a resolved one in 15, never more than 2,
# and no centre with e = 0 but one: in a layout of this coverage the neighbours of a read mostly overlap each other.
SEED, ERR = 92, 0.03
ROUNDS = 64


def _reads():
    return elba_amd.synth_reads(SEED, 60000, 12, 3000, 500, error_rate=ERR, min_len=400)


def _build():
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "elba_amd", "hostcpp")], stdout=subprocess.DEVNULL)


def _args():
    m = util.golden_meta()["small_err"][0]
    return [BIN, FA, str(m["k"]), str(m["lower"]), str(m["upper"]), str(ROUNDS)]


def test_stars_mirror_builds_and_fails_loudly_without_gpu():
    _build()
    p = subprocess.run(_args(), capture_output=True, text=True)
    if p.returncode == 3:
        assert "no HIP device" in p.stderr
    else:
        assert p.returncode == 0 and json.loads(p.stdout)["reads"] == 80


@pytest.mark.gpu
def test_stars_mirror_equals_the_python_binding(tmp_path):
    if not os.path.exists(BIN):
        _build()
    packed, off, lens, _ = _reads()
    fa = tmp_path / "reads.fa"
    with open(fa, "w") as f:
        for i, s in enumerate(cu.seqs_of(packed, off, lens)):
            f.write(">r%d\n%s\n" % (i, s))
    got = json.loads(subprocess.run([BIN, str(fa), "17", "2", "12", str(ROUNDS)], capture_output=True, text=True, check=True).stdout)
    e = elba_amd.Engine(17, 2, 12)
    e.set_reads(packed, off, lens)
    e.count_kmers(); e.create_kmer_matrix(); e.create_seed_matrix()
    e.align_seeds()
    e.transitive_reduction(0.65, 1000)
    st = e.resolve_stars(ROUNDS)
    g = e.export_string_graph()
    odd = np.flatnonzero(e.export_read_flags(len(lens)) & 32)
    cs = e.generate_contigs()
    s_checksum = int(((g["rows"] + 1) * 1000003 + g["cols"] * 10007 + g["vals"]["suffix"].astype(np.int64).astype(np.uint32).astype(np.int64)).sum())
    want = {k: st[k] for k in ("nnz_before", "nnz_after", "centres", "pairs0", "pairs1", "pairs2", "pairs3", "reads_removed", "entries_removed", "rounds_run")}
    want.update(reads=len(lens), s_checksum=s_checksum, read_checksum=int(((odd + 1) * 10007).sum()), host_equal=1, contigs=cs["contigs"], bases=cs["bases"],
                branches=cs["branches"])
    print("host mirror workload:", want)
    assert got == want
    assert len(odd) == st["reads_removed"] == 2 and st["pairs1"] == 2 and st["pairs2"] == 4 and st["centres"] == 6 and st["rounds_run"] == 2
    e.close()
