"""-m gpu: an Engine walked through the sequences of tests/state_cases.py; after every call each export answers "stage called out of
order" or not, as the case's valid products say.  One function holds the sequences that hold for the code before the table
(elba_amd/csrc/state.hpp) as well, another the places where a call now drops more (a tightening case refuses BEFORE any launch: it
must not be walked on code without the table, which would run the string-graph kernels on rows beyond the new matrix)."""
import ctypes as C
import os

import numpy as np
import pytest

import elba_amd
import state_cases as sc
import util
from oracle import pyoracle as po

pytestmark = pytest.mark.gpu
ERR_STATE = 5
PSEUDO = "matrix_of_old_reads"


@pytest.fixture(scope="module")
def small_err():
    m = util.golden_meta()["small_err"][0]
    return (m["k"], m["lower"], m["upper"]) + tuple(po.pack_reads(util.read_fasta(os.path.join(util.GOLDEN, "small_err.fa"))))


def _refused(call):
    """None when the call went through, the ElbaError when it answered ELBA_ERR_STATE; any other failure is the test's"""
    try:
        call()
    except elba_amd.ElbaError as err:
        assert err.status == ERR_STATE, str(err)
        return err
    return None


def _set_overlaps(e, nreads):
    ov = e.export_overlaps()                                       # this context's own alignments, loaded back as an edge list
    order = np.lexsort((ov["cols"], ov["rows"]))
    e.set_overlaps(nreads, ov["rows"][order], ov["cols"][order], ov["vals"][order])


def _contigs_ex(e, flags):
    st = elba_amd.capi.ContigStats()
    e._check(e.L.elba_generate_contigs_ex(e.h, C.byref(elba_amd.capi.ContigCfg(flags)), C.byref(st)))


def _actions(e, packed, off, lens):
    return {
        "set_reads": lambda: e.set_reads(packed, off, lens),
        "count_kmers": e.count_kmers, "create_kmer_matrix": e.create_kmer_matrix, "create_seed_matrix": e.create_seed_matrix,
        "align_seeds": e.align_seeds, "read_pileup": e.read_pileup, "trim_reads": e.trim_reads, "adopt_trimmed_reads": e.adopt_trimmed_reads,
        "prune_reads": lambda: e.prune_reads(1), "set_overlaps": lambda: _set_overlaps(e, len(lens)),
        "transitive_reduction": lambda: e.transitive_reduction(0.0, 1000), "generate_contigs": lambda: e.generate_contigs(singletons=True),
        "clip_tips": lambda: e.clip_tips(10, 4),
        # a hand-made 3 x 4 matrix: fewer rows than the reads the alignments were computed on
        "set_kmer_matrix": lambda: e.set_kmer_matrix(3, 4, [0, 0, 1, 1, 2, 2], [0, 1, 1, 2, 2, 3], [5, 9, 3, 7, 1, 4]),
        "clip_tips:reject": lambda: e.clip_tips(0), "generate_contigs:reject": lambda: _contigs_ex(e, 0x100),
        "read_pileup:reject": lambda: e.read_pileup(mode=2), "trim_reads:reject": lambda: e.trim_reads(min_len=0),
    }


def _probe(e, packed, lens):
    """the products whose exports do not answer ELBA_ERR_STATE, and the contig counters: (count, whether they answer at all)"""
    exports = {"reads": lambda: e.export_reads(4 * len(lens), 2 * len(packed)), "A": e.export_kmer_matrix, "B": lambda: e.export_csr(0, 0),
               "aln": e.export_overlaps, "S": e.export_string_graph, "contigs": e.export_contigs, "pileup": e.export_pileup, "trim": e.export_trim_map}
    return {name for name, call in exports.items() if _refused(call) is None}, (e.get_stat("contig_count"), e.get_stat("contig_rank_us") >= 0)


def _walk(case, data, counter_everywhere):
    k, lower, upper, packed, off, lens = data
    e = elba_amd.Engine(k, lower, upper)
    act = _actions(e, packed, off, lens)
    steps = sc.CASES[case]["steps"]
    ncontigs = None
    for i, (call, valid) in enumerate(steps):
        event, _, ending = call.partition(":")
        if event == PSEUDO:
            continue
        if ending == "":
            st = act[event]()
            if event == "generate_contigs":
                ncontigs = st["contigs"]
        elif ending == "reject":
            with pytest.raises(elba_amd.ElbaError) as err:
                act[call]()
            assert err.value.status == 1, (case, call, str(err.value))                 # ELBA_ERR_INVALID_ARG
        else:
            assert ending == "state"
            assert _refused(act[event]) is not None, (case, call)                      # refused for the state, with good arguments
        if i + 1 < len(steps) and steps[i + 1][0] == PSEUDO:
            valid = steps[i + 1][1]                                                    # (what the call does to a matrix of the old reads is part of it)
        valid = set(valid.split())
        want = {p for p in ("reads", "A", "B", "aln", "S", "pileup", "trim") if p in valid} | ({"contigs"} if {"S", "contigs"} <= valid else set())
        got, (count, counted) = _probe(e, packed, lens)
        print(case, call, sorted(got), count, counted)
        assert got == want, (case, call, sorted(got), sorted(want))
        # the counters answer like the contig exports: the last call's count, or 0 (and no rank time).  Before the table they went by the
        # contigs' own flag alone, which could outlive S, so without S only the tightening cases look at them
        if counter_everywhere or "S" in valid:
            assert (count, counted) == ((ncontigs, True) if "contigs" in want else (0, False)), (case, call, count, counted, ncontigs)
    e.close()


def test_exports_follow_the_cases_as_before_the_table(small_err):
    for case in sorted(sc.CASES):
        if sc.CASES[case].get("gpu", True) and not sc.CASES[case].get("tightening", False):
            _walk(case, small_err, counter_everywhere=False)


def test_exports_follow_the_tightened_cases(small_err):
    for case in sorted(sc.CASES):
        if sc.CASES[case].get("gpu", True) and sc.CASES[case].get("tightening", False):
            _walk(case, small_err, counter_everywhere=True)


def test_retired_options_are_unknown_names():
    """elba_set_option answers the retired switches "tune0", "tune6" and "msd_no_emit8" like any unknown name; the tuneN still read are taken"""
    e = elba_amd.Engine(17, 2, 8)
    try:
        for name in ("tune0", "tune6", "tune8", "msd_no_emit8", "no_such_option"):
            with pytest.raises(elba_amd.ElbaError) as err:
                e.set_option(name, 1)
            assert err.value.status == 1, (name, str(err.value))                       # ELBA_ERR_INVALID_ARG
        for name in ("tune1", "tune2", "tune3", "tune4", "tune5", "tune7"):
            e.set_option(name, 1)
            e.set_option(name, 0)
    finally:
        e.close()
