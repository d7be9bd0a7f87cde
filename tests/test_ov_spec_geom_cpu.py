"""Which reads-path kernel the overlap SpGEMM's plan picks — compiled geometry for columns padded to 8 entries, run-time geometry for every other stride and
under option "ov_generic" = 2 — and the claim limits the compiled-geometry kernels hold as constants (csrc/ov_plan.hpp: ov_spec_geom_ok, ov_tier_limit),
walked by a host program built with the address and undefined-behaviour sanitizers (elba_amd/hostcpp/test_ov_spec_geom.cpp): no library, no GPU."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "elba_amd", "hostcpp", "test_ov_spec_geom")


def test_ov_spec_geom_selection_and_limits():
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "elba_amd", "hostcpp"), BIN], stdout=subprocess.DEVNULL)
    p = subprocess.run([BIN], capture_output=True, text=True)
    assert p.returncode == 0 and p.stderr == "", (p.stdout[-2000:], p.stderr[-2000:])
    last = p.stdout.strip().splitlines()[-1].split()
    assert last[0] == "ok" and int(last[1]) > 100, p.stdout[-2000:]
