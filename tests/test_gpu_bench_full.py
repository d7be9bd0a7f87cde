"""`bench.py` on one GPU, plain and with `--full`: a plain run prints the headline and what its timed steps measured, and leaves every leg that
takes runs of its own (steady state, forced HBM-table tier, spgemm_prep / from_triples, CPU baselines and the oracle's parity) to `--full`,
which still runs them.  Both runs build the same matrix."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FULL_ONLY = ("steady_state", "hbm_tier_forced", "spgemm_prep", "from_triples", "cpu_baseline", "parity_vs_oracle_on_cpu_sample")


def _bench(*argv):
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--workload", "ecsample30x-like", "--steps", "2", "--warmup", "1"] + list(argv),
                       capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert p.returncode == 0, p.stderr[-2000:]
    return json.loads(p.stdout.strip().splitlines()[-1])


@pytest.mark.gpu
def test_plain_run_leaves_the_extra_legs_to_full():
    plain = _bench()
    assert plain["full"] is False and plain["value"] > 0 and plain["ms_per_step"] > 0 and plain["counts_match_one_gpu"] is True
    assert plain["unit"] == "overlap nnz/s" and plain["higher_is_better"] is True and plain["dtype"] == "u32"
    assert plain["roofline"]["algorithmic_bytes_per_step"] > 0 and plain["kmer_stage"]["instances"] == plain["counts"]["kmer_instances"]
    assert all(plain[key] is None for key in FULL_ONLY), {key: plain[key] for key in FULL_ONLY}

    full = _bench("--full", "--no-cpu-full", "--steady-steps", "2")
    assert full["full"] is True and full["counts"] == plain["counts"] and full["counts_match_one_gpu"] is True
    assert full["steady_state"]["ms_per_step"] > 0
    assert full["hbm_tier_forced"]["same_nnz_and_products"] is True and full["from_triples"]["same_nnz_and_products"] is True
    assert "spgemm_prep_ms" in full["spgemm_prep"] or "skipped" in full["spgemm_prep"]
    assert full["parity_vs_oracle_on_cpu_sample"] is True and full["cpu_baseline"]["value"] > 0
