"""The decisions of the CSR build of A — the sort-key layout of its three producers, the hand-off, the build's plan, the format of a row entry and the column
store's geometry (csrc/csr_plan.hpp) — walked by a host program built with the address and undefined-behaviour sanitizers
(elba_amd/hostcpp/test_csr_plan.cpp): no library, no GPU."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "elba_amd", "hostcpp", "test_csr_plan")


def test_csr_plan_layouts_plans_and_round_trips():
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "elba_amd", "hostcpp"), BIN], stdout=subprocess.DEVNULL)
    p = subprocess.run([BIN], capture_output=True, text=True)
    assert p.returncode == 0 and p.stderr == "", (p.stdout[-2000:], p.stderr[-2000:])
    last = p.stdout.strip().splitlines()[-1].split()
    assert last[0] == "ok" and int(last[1]) > 100000, p.stdout[-2000:]
