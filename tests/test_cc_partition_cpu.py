"""The greedy assignment of components to parts (csrc/cc_partition.hpp), walked by a host program built with the address and
undefined-behaviour sanitizers (elba_amd/hostcpp/test_cc_partition.cpp) — no library, no GPU — and the same header against the Python
restatement of the reference's loop (comp_util.partition) on random lists."""
import os
import subprocess

import numpy as np

import comp_util as ku

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "elba_amd", "hostcpp", "test_cc_partition")


def _build():
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "elba_amd", "hostcpp"), BIN], stdout=subprocess.DEVNULL)


def test_cc_partition_against_the_literal_loop_under_the_sanitizers():
    _build()
    p = subprocess.run([BIN], capture_output=True, text=True)
    assert p.returncode == 0 and p.stderr == "", (p.stdout[-2000:], p.stderr[-2000:])
    last = p.stdout.strip().splitlines()[-1].split()
    assert last[0] == "ok" and int(last[1]) > 100000, p.stdout[-2000:]


def test_cc_partition_equals_the_python_restatement():
    _build()
    rng = np.random.default_rng(5)
    for it in range(30):
        n = int(rng.integers(1, 80))
        reads = rng.integers(1, 7, n)
        weight = reads if it % 2 else rng.integers(0, (4, 1000, 1 << 40)[it % 3], n)
        nparts, min_reads = int(rng.integers(1, 70 if it % 5 == 0 else 9)), int(rng.integers(0, 4))
        text = "".join("%d %d\n" % (r, w) for r, w in zip(reads, weight))
        p = subprocess.run([BIN, str(nparts), str(min_reads)], input=text, capture_output=True, text=True)
        assert p.returncode == 0 and p.stderr == "", p.stderr[-2000:]
        lines = p.stdout.splitlines()
        poc, pw = ku.partition(reads, weight, nparts, min_reads)
        assert [int(x) for x in lines[0].split()] == poc.tolist() and [int(x) for x in lines[1].split()] == pw.tolist()
