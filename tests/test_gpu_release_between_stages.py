"""-m gpu: elba_release_workspace between the late stages.  Every stage keeps its results and gives back its scratch: a context that
releases its workspace after every call of the whole late pipeline must end with the results of a context that never releases — a result
freed as scratch shows as a difference (or a fault), and a stage that needs scratch of an earlier call finds it gone."""
import numpy as np
import pytest

import bridge_util
import bubble_util
import consensus_util as cs
import contig_util as cu
import elba_amd
import gfa_util
import placement_util as pu
import star_util
import tip_util
import trim_util
import weak_util

pytestmark = pytest.mark.gpu

# the counters of the stages whose helper module has no STATS of its own (the tuples of test_gpu_pileup.py, test_gpu_pileup_edges.py and
# test_gpu_contigs.py)
PILEUP_STATS = ("nreads", "pairs", "intervals", "segments", "max_depth", "unsupported", "split", "trimmed", "trimmed_bases")
SG_STATS = ("bad_reads", "contained_reads", "edges_kept", "products", "marked", "removed", "nnz")
CONTIG_STATS = ("nreads", "branches", "components", "used_components", "contigs", "cycles", "contig_reads", "bases", "longest")


def _only(stats, keys):
    return {k: stats[k] for k in keys}


def _tail(e, between):
    """calls 12 to 14, between() after each: the links, the placements, the polished contigs and the three calls' counters"""
    links, gst = e.assembly_links(); between()
    pl, pst = e.place_reads(); between()
    out, ost = e.polish_contigs(votes=True); between()
    return dict(links=links, pl=pl, out=out, stats=dict(links=_only(gst, gfa_util.STATS), place=_only(pst, pu.STATS), polish=_only(ost, cs.STATS)))


def _pipeline(seqs, pairs, releases):
    e = elba_amd.Engine(17, 2, 8)
    between = e.release_workspace if releases else (lambda: None)
    st = {}
    e.set_reads(*cu.pack(seqs)); between()
    e.set_overlaps(len(seqs), *pairs); between()
    st["pileup"] = _only(e.read_pileup(mode=0, margin=0, min_depth=1, min_run=1, trim_len=0), PILEUP_STATS); between()
    st["trim"] = _only(e.trim_reads(), trim_util.STATS); between()
    st["reduction"] = _only(e.transitive_reduction(0.0, 0), SG_STATS); between()
    st["tips"] = _only(e.clip_tips(3), tip_util.STATS); between()
    st["bubbles"] = _only(e.pop_bubbles(3), bubble_util.STATS); between()
    st["weak"] = _only(e.cut_weak_overlaps(), weak_util.STATS); between()
    st["bridges"] = _only(e.cut_bridges(2, 3), bridge_util.STATS); between()      # (the smallest flank the call takes for bridges of two reads)
    st["stars"] = _only(e.resolve_stars(), star_util.STATS); between()
    st["contigs"] = _only(e.generate_contigs(circular=True, singletons=True), CONTIG_STATS); between()
    return e, st, _tail(e, between)


def _resident(e, M):
    """what the stages keep on the device, exported"""
    contigs = e.export_contigs()
    return dict(pileup=e.export_pileup(), trim_map=e.export_trim_map(), trimmed=e.export_trimmed_reads(), graph=e.export_string_graph(), flags=e.export_read_flags(M),
                contigs=contigs, kinds=e.export_contig_kinds(contigs["n"]), read_contigs=e.export_read_contigs(M))


def _same_arrays(a, b):
    if isinstance(a, dict):
        return a.keys() == b.keys() and all(_same_arrays(a[k], b[k]) for k in a)
    if isinstance(a, tuple):
        return len(a) == len(b) and all(_same_arrays(x, y) for x, y in zip(a, b))
    if isinstance(a, np.ndarray):
        return a.dtype == b.dtype and np.array_equal(a, b)
    return a == b


def _assert_same_tail(a, b):
    assert gfa_util.same_records(a["links"], b["links"])
    assert pu.same_placements(a["pl"], b["pl"]), pu.first_difference(a["pl"], b["pl"])
    assert cs.first_difference(a["out"], b["out"]) is None, cs.first_difference(a["out"], b["out"])
    assert a["stats"] == b["stats"]


def test_release_after_every_call_changes_no_result():
    t = pu.truth_set(np.random.default_rng(2), 1200, 9, True, 80, 8)
    seqs, _ = cs.mutate_truth(t, np.random.default_rng(1002), 14)
    M = len(seqs)
    ea, sta, taila = _pipeline(seqs, t["pairs"], releases=True)
    eb, stb, tailb = _pipeline(seqs, t["pairs"], releases=False)
    assert taila["stats"]["place"]["nreads"] == M and len(taila["out"]["seqs"]) >= 1      # the late stages had something to do
    ra, rb = _resident(ea, M), _resident(eb, M)
    for k in ra:
        assert _same_arrays(ra[k], rb[k]), k
    assert sta == stb
    _assert_same_tail(taila, tailb)
    # once more from a released workspace: the three calls that read the contigs find them as they were
    ea.release_workspace()
    _assert_same_tail(_tail(ea, ea.release_workspace), tailb)
    assert _same_arrays(_resident(ea, M), rb)
    ea.close(); eb.close()
