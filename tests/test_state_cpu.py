"""The validity table of a context (elba_amd/csrc/state.hpp) against tests/state_cases.py, through the stand-alone program
elba_amd/hostcpp/test_state_table: no library, no GPU; the program is built with the address and undefined-behaviour sanitizers."""
import os
import subprocess

import pytest

import state_cases as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOSTCPP = os.path.join(ROOT, "elba_amd", "hostcpp")
BIN = os.path.join(HOSTCPP, "test_state_table")


@pytest.fixture(scope="module")
def table():
    subprocess.check_call(["make", "-C", HOSTCPP, BIN], stdout=subprocess.DEVNULL)
    return BIN


def _walk(binary, calls):
    p = subprocess.run([binary] + calls, capture_output=True, text=True)
    assert p.returncode == 0 and p.stderr == "", (p.returncode, p.stderr)          # (a sanitizer report lands on stderr)
    lines = [l.split() for l in p.stdout.splitlines()]
    assert [l[0] for l in lines] == calls
    for l in lines:
        assert int(l[1], 16) == sum(1 << sc.PRODUCTS.index(name) for name in l[2:])    # the names are the mask
    return [set(l[2:]) for l in lines]


@pytest.mark.parametrize("case", sorted(sc.CASES))
def test_every_step_leaves_the_products_the_case_names(table, case):
    steps = sc.CASES[case]["steps"]
    got = _walk(table, [call for call, _ in steps])
    for (call, want), have in zip(steps, got):
        assert have == set(want.split()), (case, call, sorted(have), want)


def test_the_cases_cover_what_they_must(table):
    events = subprocess.run([table, "--events"], capture_output=True, text=True, check=True).stdout.split()
    assert len(events) == len(set(events)) >= 25
    calls = {call for c in sc.CASES.values() for call, _ in c["steps"]}
    assert {call.split(":")[0] for call in calls} <= set(events)
    # a rejected call of each of the four that differ in what a rejection leaves, and the three re-entries after a full run
    assert {"clip_tips:reject", "generate_contigs:reject", "read_pileup:reject", "trim_reads:reject"} <= calls
    for event in ("set_overlaps", "set_reads", "set_kmer_matrix"):
        assert any([call for call, _ in c["steps"]][len(sc.FULL)] == event for c in sc.CASES.values() if c["steps"][:len(sc.FULL)] == sc.FULL), event
    for want in sc.PRODUCTS:
        assert any(want in valid.split() for c in sc.CASES.values() for _, valid in c["steps"])


def test_unknown_events_and_endings_are_refused(table):
    for bad in ("no_such_call", "set_reads:sometimes"):
        p = subprocess.run([table, "set_reads", bad], capture_output=True, text=True)
        assert p.returncode == 2 and "unknown event or ending" in p.stderr
