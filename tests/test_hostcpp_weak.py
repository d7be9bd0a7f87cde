"""The C++ host mirror of cutting weak overlaps (CutWeakOverlaps in elba_amd/hostcpp/elba_host.hpp) against the Python binding on one
workload: the same stats, the same cut S (checksum), the same contigs' counts, and the host's own comparison of the cut S with what the rule
keeps of the uncut one."""
import json
import os
import subprocess

import numpy as np
import pytest

import contig_util as cu
import elba_amd
import util

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "elba_amd", "hostcpp", "test_host_weak")
FA = os.path.join(util.GOLDEN, "small_err.fa")
MIN_RATIO = 0.9
Q16 = int(round(MIN_RATIO * 65536))


def _build():
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "elba_amd", "hostcpp")], stdout=subprocess.DEVNULL)


def _args():
    m = util.golden_meta()["small_err"][0]
    return [BIN, FA, str(m["k"]), str(m["lower"]), str(m["upper"]), str(Q16)]


def test_weak_mirror_builds_and_fails_loudly_without_gpu():
    _build()
    p = subprocess.run(_args(), capture_output=True, text=True)
    if p.returncode == 3:
        assert "no HIP device" in p.stderr
    else:
        assert p.returncode == 0 and json.loads(p.stdout)["reads"] == 80


@pytest.mark.gpu
def test_weak_mirror_equals_the_python_binding(tmp_path):
    if not os.path.exists(BIN):
        _build()
    packed, off, lens, _ = elba_amd.synth_reads(89, 60000, 12, 3000, 500, error_rate=0.03, min_len=400)      # its string graph has read ends with two overlaps of unlike scores
    fa = tmp_path / "reads.fa"
    with open(fa, "w") as f:
        for i, s in enumerate(cu.seqs_of(packed, off, lens)):
            f.write(">r%d\n%s\n" % (i, s))
    got = json.loads(subprocess.run([BIN, str(fa), "17", "2", "12", str(Q16)], capture_output=True, text=True, check=True).stdout)
    e = elba_amd.Engine(17, 2, 12)
    e.set_reads(packed, off, lens)
    e.count_kmers(); e.create_kmer_matrix(); e.create_seed_matrix()
    e.align_seeds()
    e.transitive_reduction(0.65, 1000)
    f0 = e.export_read_flags(len(lens))
    st = e.cut_weak_overlaps(MIN_RATIO)
    g = e.export_string_graph()
    cs = e.generate_contigs()
    s_checksum = int(((g["rows"] + 1) * 1000003 + g["cols"] * 10007 + g["vals"]["suffix"].astype(np.int64).astype(np.uint32).astype(np.int64)).sum())
    want = {k: st[k] for k in ("nnz_before", "nnz_after", "branch_sides", "weak_entries", "entries_removed", "sides_emptied")}
    want.update(reads=len(lens), s_checksum=s_checksum, host_equal=1, contigs=cs["contigs"], bases=cs["bases"], branches=cs["branches"])
    print("host mirror workload:", want)
    assert got == want
    assert st["entries_removed"] > 0 and st["weak_entries"] > 0 and st["nnz_after"] < st["nnz_before"] and (e.export_read_flags(len(lens)) == f0).all()      # the graph changed, the flags did not
    e.close()
