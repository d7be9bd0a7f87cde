"""The rows of elba_pop_bubbles, elba_cut_weak_overlaps, elba_cut_bridges and elba_resolve_stars in the validity table
(elba_amd/csrc/state.hpp), through the stand-alone program elba_amd/hostcpp/test_state_table: what elba_clip_tips does to a context, each of
them does too."""
import collections
import subprocess

import pytest

import state_cases as sc
from test_state_cpu import _walk, table      # noqa: F401 (table is the fixture that builds the program)

EVERYTHING = "reads counts A B aln S contigs pileup trim"
WITHOUT_CONTIGS = "reads counts A B aln S pileup trim"

# One row per event.  word: what its case names call the call.  others: the cleaning calls that were there before it, which go on from
# the S it leaves.  place(at): where it sits among --events, at(name) being a name's position.
Row = collections.namedtuple("Row", "event word others place")
ROWS = [
    Row("pop_bubbles", "pop", ["clip_tips"], lambda at: at("pop_bubbles") == at("clip_tips") + 1),
    Row("cut_weak_overlaps", "cut", ["clip_tips"], lambda at: at("cut_weak_overlaps") == at("pop_bubbles") + 1 == at("clip_tips") + 2),
    Row("cut_bridges", "cut", ["clip_tips", "pop_bubbles", "cut_weak_overlaps"],
        lambda at: at("cut_bridges") == at("cut_weak_overlaps") + 1 == at("generate_contigs") - 1),
    Row("resolve_stars", "call", ["clip_tips", "pop_bubbles", "cut_weak_overlaps", "cut_bridges"],
        lambda at: at("resolve_stars") == at("transitive_reduction") + 1 == at("clip_tips") - 1),
]


def cases(row):
    ev, w = row.event, row.word
    return {
        "a_rejected_%s_leaves_everything" % w: sc.FULL + [(ev + ":reject", EVERYTHING)],
        "a_%s_leaves_S_and_drops_the_contigs" % w: sc.FULL + [(ev, WITHOUT_CONTIGS), ("generate_contigs", EVERYTHING)] +
                                                   [(other, WITHOUT_CONTIGS) for other in row.others] + [(ev, WITHOUT_CONTIGS)],
        "a_%s_that_fails_in_flight_leaves_no_S" % w: sc.FULL + [(ev + ":fail", "reads counts A B aln pileup trim")],
        "without_S_it_is_refused_and_changes_nothing": sc.ALIGNED + [(ev + ":state", "reads counts A B aln")],
    }


CASES = {row.event + "-" + case: steps for row in ROWS for case, steps in cases(row).items()}


@pytest.mark.parametrize("case", sorted(CASES))
def test_cleaning_row(table, case):
    steps = CASES[case]
    got = _walk(table, [call for call, _ in steps])
    for (call, want), have in zip(steps, got):
        assert have == set(want.split()), (case, call, sorted(have), want)


@pytest.mark.parametrize("row", ROWS, ids=[row.event for row in ROWS])
def test_the_row_is_that_of_clip_tips_and_sits_where_it_was_put(table, row):
    events = subprocess.run([table, "--events"], capture_output=True, text=True, check=True).stdout.split()
    assert row.event in events and row.place(events.index)
    calls = [call for call, _ in sc.FULL]
    for ending in ("", ":reject", ":state", ":fail"):
        out = [_walk(table, calls + [ev + ending])[-1] for ev in ("clip_tips", row.event)]
        assert out[0] == out[1], ending
