"""CPU tests of bench.py's own logic: argument checks, and --dump-outputs (dump_outputs) against a stand-in for the engine that serves a
known B through the same calls (device_view, export_csr).  The GPU run of the flag is bench.py itself."""
import os
import subprocess
import sys

import numpy as np
import pytest

import bench
from elba_amd.capi import SEED_DTYPE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class HostB:
    """A random CSR B on the host behind the two engine calls dump_outputs makes."""

    def __init__(self, M, mean_row_nnz, seed=7):
        r = np.random.default_rng(seed)
        self.rowptr = np.concatenate([[0], np.cumsum(r.poisson(mean_row_nnz, M))]).astype(np.int64)
        Y = int(self.rowptr[-1])
        self.col = r.integers(0, max(1, M), Y).astype(np.uint32)
        self.val = np.zeros(Y, SEED_DTYPE)
        for f in ("q0", "t0", "q1", "t1"):
            self.val[f] = r.integers(0, 2 ** 32, Y, dtype=np.uint64).astype(np.uint32)
        self.val["numshared"] = r.integers(2, 1000, Y)
        self.M, self.Y = M, Y

    def device_view(self):
        return {"M": self.M, "Y": self.Y, "b_rowptr": 0}

    def export_csr(self, lo, hi):
        e0, e1 = int(self.rowptr[lo]), int(self.rowptr[hi])
        return {"M": hi - lo, "Y": e1 - e0, "rowptr": self.rowptr[lo:hi + 1] - e0, "col": self.col[e0:e1].astype(np.int64), "val": self.val[e0:e1].copy()}


def _dump(monkeypatch, B, path):
    monkeypatch.setattr(bench, "host_copy", lambda ptr, n, dtype: B.rowptr[:n].astype(dtype))
    st = {key: i + 3 for i, key in enumerate(bench.DUMP_COUNTS)}
    summary = bench.dump_outputs(B, st, str(path))
    arrs = {f[:-4]: np.load(os.path.join(path, f)) for f in os.listdir(path)}
    return summary, arrs, st


@pytest.mark.parametrize("M,mean", [(200100, 493), (5000, 3), (0, 1)])
def test_dump_outputs_writes_exact_entries_of_a_seeded_row_sample_within_the_limit(monkeypatch, tmp_path, M, mean):
    B = HostB(M, mean)
    s, arrs, st = _dump(monkeypatch, B, tmp_path / "a")
    assert sorted(arrs) == sorted(["counts", "b_row_nnz"] + ["b_" + f for f in bench.DUMP_ENTRY_FIELDS])
    assert all(a.dtype == np.float64 for a in arrs.values())
    assert sum(os.path.getsize(os.path.join(tmp_path / "a", f)) for f in os.listdir(tmp_path / "a")) == s["bytes"] <= bench.DUMP_LIMIT_BYTES
    assert list(arrs["counts"]) == [st[key] for key in bench.DUMP_COUNTS]
    assert (arrs["b_row_nnz"] == np.diff(B.rowptr)).all()
    rows = np.unique(arrs["b_row"]).astype(np.int64)
    assert len(rows) <= s["rows_sampled"] and (np.diff(arrs["b_row"]) >= 0).all()          # (rows without entries leave no trace in b_row)
    idx = np.concatenate([np.arange(B.rowptr[r], B.rowptr[r + 1]) for r in rows] + [np.zeros(0, np.int64)])
    assert len(idx) == s["entries_sampled"] == len(arrs["b_col"])
    assert (arrs["b_col"] == B.col[idx]).all()
    for f in bench.DUMP_ENTRY_FIELDS[2:]:
        assert (arrs["b_" + f] == B.val[f][idx]).all(), f
    if B.Y * 8 * len(bench.DUMP_ENTRY_FIELDS) < bench.DUMP_LIMIT_BYTES // 2:
        assert s["rows_sampled"] == M and (rows == np.flatnonzero(np.diff(B.rowptr))).all()  # all of B when it fits
    s2, arrs2, _ = _dump(monkeypatch, B, tmp_path / "b")                   # the same B gives the same files
    assert s2["rows_sampled"] == s["rows_sampled"] and all((arrs2[n] == arrs[n]).all() for n in arrs)


@pytest.mark.parametrize("argv", [["--steps", "0"], ["--warmup", "-1"]])
def test_bench_rejects_steps_below_one_and_negative_warmup(argv):
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + argv, capture_output=True, text=True, timeout=120, cwd=ROOT)
    assert p.returncode == 2 and ("--steps" in p.stderr or "--warmup" in p.stderr), p.stderr
