"""CPU: the oracle's multi-threaded k-mer stage (orc_count_and_build_mt) when the OpenMP runtime delivers FEWER threads than asked for.  Every GPU
test trusts this oracle; a read or column range left without a thread would drop entries of A without a word."""
import os
import subprocess
import sys

import numpy as np
import pytest

import util
from oracle import pyoracle as po

G = util.GOLDEN
ROOT = util.ROOT

_CHILD = r"""
import sys
import numpy as np
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
import util
from oracle import pyoracle as po
packed, off, lens = po.pack_reads(util.read_fasta(sys.argv[2]))
o = po.Oracle(int(sys.argv[3]), int(sys.argv[4]), int(sys.argv[5]))
o.count_and_build(packed, off, lens, 8)
A = o.A()
arrs = {k: v for k, v in A.items() if isinstance(v, np.ndarray)}
arrs["_stats"] = np.array([o.stat(s) for s in ("I", "N", "Z", "ndistinct", "M")], dtype=np.int64)
np.savez(sys.argv[6], **arrs)
"""


@pytest.mark.parametrize("name,k,lo,up", [("small_err.fa", 17, 2, 8), ("reads_ref.fa.gz", 31, 15, 35)])
def test_the_oracle_on_fewer_threads_than_asked_for_equals_one_thread(tmp_path, name, k, lo, up):
    """A fresh process under OMP_THREAD_LIMIT=2 asks orc_count_and_build_mt for 8 threads: the read ranges and column ranges of the six threads
    that never start are walked all the same — every array of A and every counter equal the one-thread statement's."""
    path = os.path.join(G, name)
    out = str(tmp_path / "A.npz")
    env = dict(os.environ, OMP_THREAD_LIMIT="2", OMP_DYNAMIC="false")
    subprocess.run([sys.executable, "-c", _CHILD, ROOT, path, str(k), str(lo), str(up), out], env=env, check=True, timeout=600)
    got = np.load(out)
    packed, off, lens = po.pack_reads(util.read_fasta(path))
    o = po.Oracle(k, lo, up)
    o.count_and_build(packed, off, lens)
    A = o.A()
    assert A["Z"] > 0
    for key, v in A.items():
        if isinstance(v, np.ndarray):
            assert np.array_equal(v, got[key]), key
    assert list(got["_stats"]) == [o.stat(s) for s in ("I", "N", "Z", "ndistinct", "M")]
