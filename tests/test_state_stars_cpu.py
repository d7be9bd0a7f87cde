"""The row of elba_resolve_stars in the validity table (elba_amd/csrc/state.hpp), through the stand-alone program
elba_amd/hostcpp/test_state_table: what elba_clip_tips does to a context, elba_resolve_stars does too."""
import os
import subprocess

import pytest

import state_cases as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOSTCPP = os.path.join(ROOT, "elba_amd", "hostcpp")
BIN = os.path.join(HOSTCPP, "test_state_table")

EVERYTHING = "reads counts A B aln S contigs pileup trim"

CASES = {
    "a_rejected_call_leaves_everything": sc.FULL + [("resolve_stars:reject", EVERYTHING)],
    "a_call_leaves_S_and_drops_the_contigs": sc.FULL + [
        ("resolve_stars", "reads counts A B aln S pileup trim"),
        ("generate_contigs", EVERYTHING),
        ("clip_tips", "reads counts A B aln S pileup trim"),                         # and the other calls go on from there
        ("pop_bubbles", "reads counts A B aln S pileup trim"),
        ("cut_weak_overlaps", "reads counts A B aln S pileup trim"),
        ("cut_bridges", "reads counts A B aln S pileup trim"),
        ("resolve_stars", "reads counts A B aln S pileup trim"),
    ],
    "a_call_that_fails_in_flight_leaves_no_S": sc.FULL + [("resolve_stars:fail", "reads counts A B aln pileup trim")],
    "without_S_it_is_refused_and_changes_nothing": sc.ALIGNED + [("resolve_stars:state", "reads counts A B aln")],
}


@pytest.fixture(scope="module")
def table():
    subprocess.check_call(["make", "-C", HOSTCPP, BIN], stdout=subprocess.DEVNULL)
    return BIN


@pytest.mark.parametrize("case", sorted(CASES))
def test_resolve_stars_row(table, case):
    steps = CASES[case]
    calls = [call for call, _ in steps]
    p = subprocess.run([table] + calls, capture_output=True, text=True)
    assert p.returncode == 0 and p.stderr == "", (p.returncode, p.stderr)            # (a sanitizer report lands on stderr)
    lines = [l.split() for l in p.stdout.splitlines()]
    assert [l[0] for l in lines] == calls
    for (call, want), l in zip(steps, lines):
        assert int(l[1], 16) == sum(1 << sc.PRODUCTS.index(name) for name in l[2:])
        assert set(l[2:]) == set(want.split()), (case, call, l[2:], want)


def test_the_row_is_clip_tips_and_sits_between_the_reduction_and_clip_tips(table):
    events = subprocess.run([table, "--events"], capture_output=True, text=True, check=True).stdout.split()
    assert "resolve_stars" in events and events.index("resolve_stars") == events.index("transitive_reduction") + 1 == events.index("clip_tips") - 1
    calls = [call for call, _ in sc.FULL]
    for ending in ("", ":reject", ":state", ":fail"):
        out = [subprocess.run([table] + calls + [ev + ending], capture_output=True, text=True, check=True).stdout.splitlines()[-1].split()[1:]
               for ev in ("clip_tips", "resolve_stars")]
        assert out[0] == out[1], ending
