"""What the tests of the C++ host mirror's self-test programs (elba_amd/hostcpp/test_host_*.cpp) share: building a program, running it for
its JSON line, and the Python side of the checksums that elba_amd/hostcpp/host_test.hpp computes."""
import json
import os
import subprocess

import numpy as np

import elba_amd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOSTCPP = os.path.join(ROOT, "elba_amd", "hostcpp")
_built = {}


def binary(name):
    """The path of the program `name`, built (or found up to date) once per process."""
    if name not in _built:
        path = os.path.join(HOSTCPP, name)
        subprocess.check_call(["make", "-C", HOSTCPP, path], stdout=subprocess.DEVNULL)
        _built[name] = path
    return _built[name]


def run_json(bin, args, **env):
    """Runs the program, which must succeed, and returns its output, one line of JSON; env adds to the environment."""
    p = subprocess.run([bin] + [str(a) for a in args], capture_output=True, text=True, env=dict(os.environ, **env))
    assert p.returncode == 0, p.stderr
    return json.loads(p.stdout)


def runs_or_reports_no_device(args):
    """The program args[0] with its arguments: the JSON it prints, or None after it said loudly that there is no GPU (no silent CPU path)."""
    p = subprocess.run([str(a) for a in args], capture_output=True, text=True)
    if p.returncode == 3:
        assert "no HIP device" in p.stderr
        return None
    assert p.returncode == 0, p.stderr
    return json.loads(p.stdout)


def write_fasta(path, seqs):
    with open(path, "w") as f:
        for i, s in enumerate(seqs):
            f.write(">r%d\n%s\n" % (i, s))
    return path


def s_checksum(g):
    """host_test.hpp's s_checksum on an exported string graph"""
    return int(((g["rows"] + 1) * 1000003 + g["cols"] * 10007 + g["vals"]["suffix"].astype(np.int64).astype(np.uint32).astype(np.int64)).sum())


def read_checksum(reads):
    """host_test.hpp's read_checksum on an array of read ids"""
    return int(((reads + 1) * 10007).sum())


def pipeline_engine(packed, off, lens, k, lo, up):
    """An engine taken through the binding as far as run_to_string_graph takes the mirror: reads to transitive_reduction(0.65, 1000)."""
    e = elba_amd.Engine(k, lo, up)
    e.set_reads(packed, off, lens)
    e.count_kmers(); e.create_kmer_matrix(); e.create_seed_matrix()
    e.align_seeds()
    e.transitive_reduction(0.65, 1000)
    return e
