"""The plan of the k-mer stage's two-level partition and the planners of its value-range passes (csrc/msd_plan.hpp), walked by a host program built
with the address and undefined-behaviour sanitizers (elba_amd/hostcpp/test_msd_plan.cpp): no library, no GPU."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "elba_amd", "hostcpp", "test_msd_plan")


def test_msd_plan_and_pass_planners():
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "elba_amd", "hostcpp"), BIN], stdout=subprocess.DEVNULL)
    p = subprocess.run([BIN], capture_output=True, text=True)
    assert p.returncode == 0 and p.stderr == "", (p.stdout[-2000:], p.stderr[-2000:])
    last = p.stdout.strip().splitlines()[-1].split()
    assert last[0] == "ok" and int(last[1]) > 10000, p.stdout[-2000:]
