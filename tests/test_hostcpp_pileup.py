"""The C++ host mirror of the pileup stage (GetReadPileup, PileupVector::GetTrimmedInterval, PruneFull in elba_amd/hostcpp/elba_host.hpp)
against the Python binding on one workload: the same pileups (per-base checksum), the host trim equal to the device's on every read, the
same prune and string graph."""
import os

import numpy as np
import pytest

import elba_amd
import hostcpp_util as hu
import util
from oracle import pyoracle as po

FA = os.path.join(util.GOLDEN, "small_err.fa")
CFG = dict(mode=1, margin=20, min_depth=2, min_run=300, trim_len=500)
MASK = 3


def _args():
    m = util.golden_meta()["small_err"][0]
    return [hu.binary("test_host_pileup"), FA, str(m["k"]), str(m["lower"]), str(m["upper"])] + [str(CFG[k]) for k in ("mode", "margin", "min_depth", "min_run", "trim_len")] + [str(MASK)]


def test_pileup_mirror_builds_and_fails_loudly_without_gpu():
    got = hu.runs_or_reports_no_device(_args())
    assert got is None or got["reads"] == 80


@pytest.mark.gpu
def test_pileup_mirror_equals_the_python_binding():
    args = _args()
    got = hu.run_json(args[0], args[1:])
    m = util.golden_meta()["small_err"][0]
    packed, off, lens = po.pack_reads(util.read_fasta(FA))
    e = elba_amd.Engine(m["k"], m["lower"], m["upper"])
    e.set_reads(packed, off, lens)
    e.count_kmers(); e.create_kmer_matrix(); e.create_seed_matrix()
    e.align_seeds()
    st = e.read_pileup(**CFG)
    p = e.export_pileup()
    checksum, base = 0, 0
    for v in range(p["n"]):
        a, b = int(p["seg_off"][v]), int(p["seg_off"][v + 1])
        ends = np.concatenate([p["seg_start"][a + 1:b], [lens[v]]]).astype(np.int64)
        d = np.repeat(p["seg_depth"][a:b].astype(np.int64), ends - p["seg_start"][a:b])
        w = (np.arange(base, base + len(d), dtype=np.int64) % 1000003) + 1
        checksum += int((d * w).sum())
        base += len(d)
    flagged = int(((p["flags"] & MASK) != 0).sum())
    kept = e.prune_reads(MASK)
    sst = e.transitive_reduction(0.65, 1000)
    want = {"reads": 80, "pairs": st["pairs"], "segments": st["segments"], "pileup_checksum": checksum % (1 << 64), "trim_equal": 1,
            "flagged": flagged, "kept": kept, "string_nnz": sst["nnz"]}
    assert got == want
    assert st["pairs"] > 0 and st["segments"] > 80
    e.close()
