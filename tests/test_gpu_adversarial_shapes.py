"""-m gpu: inputs shaped to reach the corners of the k-mer stage and the SpGEMM's tier schedule that ordinary read sets miss — a crowded bucket of the
wide partition with few kept entries next to ordinary buckets, one first digit that holds most of the input under value-range batching, and rows
forwarded past the matrix's guaranteed tier on a cold call.  Each test proves from a diagnostic counter that its input reaches the shape, then
compares with the CPU oracle entry for entry."""
import numpy as np
import pytest

import elba_amd
import gpu_util as gu
import synth
from oracle import pyoracle as po

pytestmark = pytest.mark.gpu

_BASES = np.frombuffer(b"ACGT", dtype=np.uint8)


def _random_seqs(rng, n, length):
    return [t.tobytes() for t in _BASES[rng.integers(0, 4, size=(n, length))]]


def _counts_equal(ks, o):
    assert (ks["instances"], ks["distinct"], ks["reliable"], ks["entries"]) == (o.stat("I"), o.stat("ndistinct"), o.stat("N"), o.stat("Z"))


def _same_matrices(a, b):
    gu.assert_A_equal(a[0], b[0])
    gu.assert_B_equal(a[1], b[1])


# ---- 1. a crowded bucket of the wide partition (k = 31) whose folded entry count lies in an emit class -------------------------------------------
# k31_count gives up a bucket of more than 3072 distinct k-mers: its entries are never written to the partition buffer, its pseudo-buckets are counted
# and emitted on their own.  The main emit kernels must not take the parent, whatever its folded entry count.

def _satellite(rng, lead, tail_len, trail, n_single, n_rep):
    """31-mers of one leading run: n_single of them once, n_rep of them 2-4 times (the reliable ones: LOWER = 2, UPPER = 8)."""
    kms = [lead + t + trail for t in _random_seqs(rng, n_single + n_rep, tail_len)]
    reps = rng.integers(2, 5, size=n_rep)
    return kms[:n_single] + [s for s, c in zip(kms[n_single:], reps) for _ in range(int(c))]


# where: the crowded parent is the lowest bucket (ten A: canonical = forward) or a middle one (C + nine A ... GG: the reverse complement starts with CC);
# zclass: its folded entry count in 1..2048 / 2049..4096 / 4097..8192 (then with an ordinary bucket of that class, so the 1024-lane class launches)
_LEAD = {"lowest": (b"A" * 10, 21, b""), "middle": (b"C" + b"A" * 9, 19, b"GG")}
_ZCLASS = {1: (300, 0, 2048), 2: (1000, 2048, 4096), 3: (1700, 4096, 8192)}


@pytest.mark.parametrize("where,zclass,bits", [("lowest", 1, 0), ("middle", 1, 0), ("lowest", 2, 0), ("middle", 2, 0), ("middle", 3, 0), ("lowest", 3, 0),
                                               ("lowest", 1, 10), ("middle", 2, 10)])
def test_crowded_wide_bucket_with_few_kept_entries_next_to_ordinary_buckets(where, zclass, bits):
    """Error-rich k = 31 reads plus one bucket of > 3072 distinct 31-mers, most of them singletons: a crowded parent whose folded entry count
    falls in a class the main emit kernels launch.  kmer_crowded_small proves the shape; counts, A, B and the statistics equal the oracle's, and two
    more runs on the same engine are bit-identical to the first (a race against a neighbour's emit would show as a run-to-run difference)."""
    k, lo, up = 31, 2, 8
    rng = np.random.default_rng(1000 + 10 * zclass + bits + (1 if where == "middle" else 0))
    reads, _ = synth.make_reads(31 + zclass, 100000, 10, 2000, 500, error=0.10, min_len=100)
    n_rep, zlo, zhi = _ZCLASS[zclass]
    lead, tail_len, trail = _LEAD[where]
    extra = _satellite(rng, lead, tail_len, trail, 3500, n_rep)
    if zclass == 3:      # an ORDINARY bucket of 4097..8192 entries: G + nine A ... CC, 700 distinct 31-mers seven times each
        extra += [s for s in (b"G" + b"A" * 9 + t + b"CC" for t in _random_seqs(rng, 700, 19)) for _ in range(7)]
    seqs = list(reads) + extra
    np.random.default_rng(5).shuffle(seqs)
    packed, off, lens = po.pack_reads(seqs)
    o = gu.oracle_run(packed, off, lens, k, lo, up, threads=8)
    # the parent's folded entry count, from the oracle's columns: the bucket is the leading T bits of the k-mers' left-aligned values (the split
    # the library picks for I)
    T = bits
    if T == 0:
        T = 12
        while T < 20 and (o.stat("I") >> T) > 512:
            T += 1
    oA = o.A()
    ccount = np.diff(oA["colptr"])
    lead_val = 0
    for x in lead:
        lead_val = lead_val * 4 + b"ACGT".index(x)
    parent = (lead_val << (2 * (32 - len(lead)))) >> (64 - T)
    zpar = int(ccount[(oA["kmers"] >> np.uint64(64 - T)) == np.uint64(parent)].sum())
    assert zlo < zpar <= zhi, (zpar, zlo, zhi)

    e = elba_amd.Engine(k, lo, up, options={"kmer_msd": 1, "msd_wide_bits": bits})
    e.set_reads(packed, off, lens)
    runs = []
    for rep in range(3):
        ks = e.count_kmers()
        e.create_kmer_matrix()
        st = e.create_seed_matrix()
        assert e.get_stat("kmer_path") == 2
        assert e.get_stat("kmer_crowded_buckets") >= 1 and e.get_stat("kmer_crowded_small") >= 1
        _counts_equal(ks, o)
        gu.assert_stats_equal(st, o)
        runs.append((e.export_kmer_matrix(), e.export_csr()))
        if rep == 0:
            gu.assert_A_equal(runs[0][0], oA)
            gu.assert_B_equal(runs[0][1], o.B())
        else:
            _same_matrices(runs[rep], runs[0])
    e.close()


# ---- 2. one dominant first digit under value-range batching (k = 17) ----------------------------------------------------------------------------
# A pass takes whole first digits: a digit that alone holds most of the input is a pass larger than any cap.  The partition buffers must hold it.

def _dominant_digit_reads():
    reads, _ = synth.make_reads(211, 120000, 9, 3000, 800, error=0.05, min_len=100)
    poly = [b"A" * 1016] * 5000                                         # 5 M instances of the k-mer 0 (never kept: more than UPPER copies)
    return list(reads) + poly, 5000 * (1016 - 17 + 1)


def _at_rich_reads():
    reads, _ = synth.make_reads(212, 120000, 9, 3000, 800, error=0.05, min_len=100)
    rng = np.random.default_rng(213)
    g = np.where(rng.random(200000) < 0.01, rng.choice(np.frombuffer(b"CG", dtype=np.uint8), 200000), rng.choice(np.frombuffer(b"AT", dtype=np.uint8), 200000))
    gb = g.astype(np.uint8).tobytes()
    starts = rng.integers(0, 200000 - 5000, size=200)
    return list(reads) + [gb[s:s + 5000] for s in starts], 0


@pytest.mark.parametrize("shape,up", [("poly_a", 8), ("poly_a", 40), ("at_rich", 8), ("at_rich", 40)])
def test_value_range_batches_hold_a_dominant_first_digit(shape, up):
    """Ordinary reads plus 5 M instances of the k-mer 0 (poly-A reads): one first digit holds more than I/2 + 2^20 + 1 instances — more than the
    passes' buffers once held, whatever the first digit's width — and is one pass of its own.  Batched one pass per digit, and with a cap of a
    third of the instances, counts, A, B and the statistics equal the unbatched run's and the oracle's.  AT-rich reads (random A/T with rare C/G): no k-mer dominates,
    but a few digits hold most instances — a pass larger than the cap, the same matrices."""
    k, lo = 17, 2
    seqs, n0 = (_dominant_digit_reads if shape == "poly_a" else _at_rich_reads)()
    packed, off, lens = po.pack_reads(seqs)
    o = gu.oracle_run(packed, off, lens, k, lo, up, threads=8)
    e0, ks0, ms0, st0 = gu.gpu_full(packed, off, lens, k, lo, up, options={"kmer_msd": 1})
    assert e0.get_stat("kmer_path") == 1 and e0.get_stat("kmer_passes") == 1
    I = int(ks0["instances"])
    assert e0.get_stat("kmer_largest_pass") == I
    _counts_equal(ks0, o)
    ref = (e0.export_kmer_matrix(), e0.export_csr())
    gu.assert_A_equal(ref[0], o.A())
    gu.assert_B_equal(ref[1], o.B())
    gu.assert_stats_equal(st0, o)
    e0.close()
    if shape == "poly_a":
        assert n0 > 1 + I // 2 + (1 << 20), (n0, I)                    # (I >> (b1 - 1) <= I / 2 for every b1 >= 2)
        caps = (1, I // 3 + 1)
    else:
        caps = (I // 100,)       # (a few first digits hold the AT-rich half of the input: one of them alone is more than 1 %)
    for cap in caps:
        e, ks, ms, st = gu.gpu_full(packed, off, lens, k, lo, up, options={"kmer_msd": 1, "kmer_batch_instances": cap})
        assert e.get_stat("kmer_path") == 1 and e.get_stat("kmer_passes") >= 2
        largest = e.get_stat("kmer_largest_pass")
        assert largest > cap and largest <= I
        if shape == "poly_a":
            assert largest >= n0
        assert all(ks[f] == ks0[f] for f in ("instances", "distinct", "reliable", "entries"))
        _same_matrices((e.export_kmer_matrix(), e.export_csr()), ref)
        gu.assert_stats_equal(st, o)
        e.close()


# ---- 3. rows forwarded past the guaranteed tier (cold call, small dense matrix) -------------------------------------------------------------------
# Without a prior, a row predicted not to fit its tier is forwarded to the tier the prediction names.  With few reads, the tiers the host launches stop
# at the one guaranteed to fit any row (distinct partners <= reads): the forwarding must stop there too.

def _deep_short_genome():
    """1000 reads of 600 bases from 2400 bases at ~250x with 4 % substitutions, both strands, and six accurate reads of 2000 bases at the end: the
    short reads' errors leave them few row entries (LOWER = 10 keeps the repeated errors out) for the partners they find, the long reads' entries
    (~1980) start them below the guaranteed tier — and the partners-per-entry ratio of the short rows predicts more partners for a long row than
    the guaranteed tier's limit."""
    rng = np.random.default_rng(4242)
    G = 2400
    genome = _BASES[rng.integers(0, 4, G)]

    def read(pos, ln, error):
        s = genome[pos:pos + ln].copy()
        err = rng.random(ln) < error
        s[err] = _BASES[rng.integers(0, 4, int(err.sum()))]
        b = s.tobytes()
        return synth.revcomp(b) if rng.random() < 0.5 else b

    seqs = [read(int(p), 600, 0.04) for p in rng.integers(0, G - 600 + 1, 1000)]
    seqs += [read(int(p), 2000, 0.0) for p in rng.integers(0, G - 2000 + 1, 6)]
    return seqs


@pytest.mark.parametrize("no_suffix", [1, 0])
def test_rows_forwarded_on_a_cold_call_stay_within_the_launched_tiers(no_suffix):
    """A fresh engine (no prior, fewer than 8192 rows: no sample) on a small, deep matrix: rows are forwarded on the in-call prediction
    (overlap_forwarded), the call takes one pass and returns ELBA_OK, B and the statistics equal the oracle's — on the general path and on the
    dense one (dense_up = 0: its rows start on the smallest tier, like the general path's, so the long rows are predicted from finished ones)."""
    k, lo, up = 17, 10, 400
    seqs = _deep_short_genome()
    assert len(seqs) < 8192
    packed, off, lens = po.pack_reads(seqs)
    opts = {"no_suffix": no_suffix}
    if not no_suffix:
        opts["dense_up"] = 0
    e, ks, ms, st = gu.gpu_full(packed, off, lens, k, lo, up, options=opts)
    assert e.get_stat("overlap_forwarded") >= 1
    assert e.get_stat("overlap_passes") == 1
    o = gu.oracle_run(packed, off, lens, k, lo, up, threads=8)
    _counts_equal(ks, o)
    gu.assert_B_equal(e.export_csr(), o.B())
    gu.assert_stats_equal(st, o)
    e.close()
