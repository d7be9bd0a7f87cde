"""The plan of the overlap SpGEMM's host driver, its tier table, the repeated pass and the hint updates (csrc/ov_plan.hpp), walked by a host program built
with the address and undefined-behaviour sanitizers (elba_amd/hostcpp/test_ov_plan.cpp): no library, no GPU."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "elba_amd", "hostcpp", "test_ov_plan")


def test_ov_plan_tier_table_and_hints():
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "elba_amd", "hostcpp"), BIN], stdout=subprocess.DEVNULL)
    p = subprocess.run([BIN], capture_output=True, text=True)
    assert p.returncode == 0 and p.stderr == "", (p.stdout[-2000:], p.stderr[-2000:])
    last = p.stdout.strip().splitlines()[-1].split()
    assert last[0] == "ok" and int(last[1]) > 100000, p.stdout[-2000:]
