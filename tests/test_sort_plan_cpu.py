"""The decisions of the k-mer stage's sort path — the one word an instance of k <= 31 travels in, the memory plan of the multi-word sort of k > 31, the
cut of the value space into passes and the pass that cannot run (csrc/sort_plan.hpp) — walked by a host program built with the address and
undefined-behaviour sanitizers (elba_amd/hostcpp/test_sort_plan.cpp): no library, no GPU."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "elba_amd", "hostcpp", "test_sort_plan")


def test_sort_plan_word_layout_capacity_and_pass_cuts():
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "elba_amd", "hostcpp"), BIN], stdout=subprocess.DEVNULL)
    p = subprocess.run([BIN], capture_output=True, text=True)
    assert p.returncode == 0 and p.stderr == "", (p.stdout[-2000:], p.stderr[-2000:])
    last = p.stdout.strip().splitlines()[-1].split()
    assert last[0] == "ok" and int(last[1]) > 100000, p.stdout[-2000:]
