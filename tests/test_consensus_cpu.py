"""CPU: the two restatements of contig polishing (consensus_util.py) against the hand cases' claims, against each other under shuffled read
orders, and on ground-truth layouts with planted errors, where the polished contig must be the genome.  The seeds of the ground-truth test
are ones for which the restatement alone recovers the truth on every set: the GPU tests compare the device with the restatements, so no
device test can hide a miss of the rule behind the generator.  Also: the library's exports and its ABI version."""
import ctypes as C
import os

import numpy as np
import pytest

import consensus_util as cs
import contig_ex_util as cx
import contig_util as cu
import placement_util as pu

HAND = cs.hand_cases()
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("case", HAND, ids=[c["name"] for c in HAND])
def test_hand_cases_hold_in_both_restatements(case):
    a, sa = cs.polish_loops(case["cin"])
    b, sb = cs.polish_tables(case["cin"])
    assert cs.first_difference(a, b) is None and sa == sb, (cs.first_difference(a, b), sa, sb)
    assert cs.check_claims(case, a, sa) is None, cs.check_claims(case, a, sa)
    assert sa["voted"] + sa["rejected"] + sa["outside"] == len(case["cin"]["seqs"])


def test_the_hand_cases_are_the_ones_the_placement_rule_gives():
    """The records a hand case writes down are those placement_util derives from the case's own graph (chain + contained reads)."""
    for case in HAND:
        seqs, lens, (rows, cols, vals), cflags = cs.pairs_of_case(case)
        chains = [[(r, p, st) for r, (_, p, st) in enumerate(case["chain"])]]
        inp = pu.inputs_of_chains(lens, chains, [case["kind"]], rows, cols, vals, None, 1)
        pl, _ = pu.place_tables(inp)
        got, want = pl["reads"], case["cin"]["reads"]
        for f in ("start", "contig", "strand", "kind", "flags"):
            assert (got[f] == want[f]).all(), (case["name"], f, got[f], want[f])


def _truth(seed, glen, nchain, circular, ncont, nextra, nerr):
    t = pu.truth_set(np.random.default_rng(seed), glen, nchain, circular, ncont, nextra)
    seqs, sites = cs.mutate_truth(t, np.random.default_rng(seed + 1000), nerr)
    M = len(seqs)
    contigs, chains, kinds, _, _ = cx.generate_contigs_ex(M, *cu.symmetric(t["edges"]), seqs, cx.CIRCULAR, t["read_flags"])
    inp = pu.inputs_of_chains(t["lens"], chains, kinds, *t["pairs"], t["read_flags"], 1)
    pl, _ = pu.place_tables(inp)
    return t, seqs, sites, contigs, kinds, pl


TRUTH = [(1, 900, 12, False, 60, 6, 12), (2, 1200, 9, True, 80, 8, 14), (5, 1500, 20, False, 110, 12, 16), (7, 600, 6, False, 45, 3, 8)]


@pytest.mark.parametrize("seed,glen,nchain,circular,ncont,nextra,nerr", TRUTH)
def test_planted_errors_are_polished_away(seed, glen, nchain, circular, ncont, nextra, nerr):
    t, seqs, sites, contigs, kinds, pl = _truth(seed, glen, nchain, circular, ncont, nextra, nerr)
    assert len(sites) >= nerr // 2 and [len(s) for s in seqs] == t["lens"] and len(contigs) == 1
    backbone = {r for r, _, _ in sites if r in t["chain_ids"]}
    cin = cs.inputs_of(seqs, contigs, kinds, pl["reads"], 64, 0.25, 3)
    a, sa = cs.polish_tables(cin)
    assert backbone and not cs.same_sequence(contigs[0], t["genome"], circular)
    assert cs.same_sequence(a["seqs"][0], t["genome"], circular), (sites, sa)
    assert sa["rejected"] == 0 and sa["voted"] == len(seqs)
    if glen <= 900:
        b, sb = cs.polish_loops(cin, np.random.default_rng(seed).permutation(len(seqs)))
        assert cs.first_difference(a, b) is None and sa == sb


@pytest.mark.parametrize("seed", [11, 12, 13])
def test_the_two_forms_agree_on_noisy_reads_in_any_order(seed):
    """Reads with 8 % random errors of all three kinds, placed with a jitter of +-3, bands 64 and 128, all three contig kinds."""
    rng = np.random.default_rng(seed)
    genome = cx.random_genome(rng, 260)
    kind = (cx.PATH, cx.CIRCLE, cx.SINGLE)[seed % 3]
    seqs, recs = [], []
    src = genome * 3
    for r in range(14):
        l = int(rng.integers(40, 120))
        a = int(rng.integers(-10, 250)) if kind != cx.CIRCLE else int(rng.integers(0, 260))
        s = list(src[260 + a:260 + a + l])
        out = []
        for ch in s:
            u = rng.random()
            if u < 0.03:
                out.append("ACGT"[int(rng.integers(0, 4))])
            elif u < 0.055:
                continue
            elif u < 0.08:
                out += [ch, "ACGT"[int(rng.integers(0, 4))]]
            else:
                out.append(ch)
        s = "".join(out) or "A"
        strand = int(rng.integers(0, 2))
        start = a + int(rng.integers(-3, 4))
        l = len(s)
        if kind == cx.CIRCLE:
            fl = (pu.CLIPPED if l > 260 else 0) | (pu.WRAPPED if start % 260 + min(l, 260) > 260 else 0)
        else:
            lo, hi = max(start, 0), min(start + l, 260)
            fl = (pu.CLIPPED if (lo, hi) != (start, start + l) else 0) | (pu.OUTSIDE if hi <= lo else 0)
        seqs.append(cu.revcomp(s) if strand else s)
        recs.append((start, 0, 0, 0, strand, pu.ANCHORED, fl, 0))
    seqs.append("ACGT"); recs.append((0, -1, 14, 0, 0, pu.NONE, 0, 0))
    reads = np.array(recs, dtype=pu.PLACEMENT)
    for band, md in ((64, 2), (128, 1)):
        cin = cs.inputs_of(seqs, [genome], [kind], reads, band, 0.3, md)
        a, sa = cs.polish_tables(cin)
        for _ in range(2):
            b, sb = cs.polish_loops(cin, rng.permutation(len(seqs)))
            assert cs.first_difference(a, b) is None and sa == sb, cs.first_difference(a, b)
        assert sa["voted"] > 8 and int(a["col"][:, 4].sum()) > 0 and int(a["gap"].sum()) > 0


def test_library_exports_and_abi_version():
    from elba_amd import capi
    assert "elba_polish_contigs" in capi.EXPORTED_SYMBOLS and "elba_free_polished" in capi.EXPORTED_SYMBOLS
    lib = C.CDLL(capi.lib_path())
    for name in ("elba_polish_contigs", "elba_free_polished"):
        assert getattr(lib, name) is not None
    lib.elba_abi_version.restype = C.c_int
    assert lib.elba_abi_version() == 3
    with open(os.path.join(ROOT, "include", "elba_amd.h")) as f:
        text = f.read()
    assert "#define ELBA_ABI_VERSION 3" in text.replace("  ", " ") or "ELBA_ABI_VERSION 3" in text
    assert C.sizeof(capi.PolishCfg) == 32 and C.sizeof(capi.PolishStats) == 88 and capi.POLISH_READ_DTYPE.itemsize == 16
