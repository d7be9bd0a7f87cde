"""-m gpu: value-range passes of the sort of two- and three-word k-mers (k > 31, kmer.hip: count_long_kmers_in_passes).  Inputs the sort cannot take
at once — 2^32 instances and more, more than the option "kmer_batch_instances", more than the device memory holds — are counted in passes over ranges
of the leading 24 bits of the canonical first word.  Every test that forces passes proves it from kmer_passes (before: the option was ignored at
k > 31, one pass), then compares with the unbatched run and the CPU oracle."""
import os
import time

import numpy as np
import pytest

import elba_amd
import gpu_util as gu
import synth
import util
from oracle import pyoracle as po

pytestmark = pytest.mark.gpu

G = util.GOLDEN
_SEED_FIELDS = ("nnz", "products", "nnz_before_prune", "nnz_diag", "nnz_upper", "max_numshared")
_COUNT_FIELDS = ("instances", "distinct", "reliable", "entries")


# ---- the canonical multi-word k-mer on the host --------------------------------------------------------------------------------------------------

def canonical_words(packed, off, reads, poss, k):
    """canonical k-mer (W = ceil(k / 32) left-aligned 64-bit words, first word most significant) at (read, pos) of every entry, from the packed
    reads (2 bits per base, first base in the high bits of its byte; A C G T = 0 1 2 3; twin = reverse complement; canonical = the smaller)."""
    reads = np.asarray(reads, dtype=np.int64)
    poss = np.asarray(poss, dtype=np.int64)
    W = (k + 31) // 32
    out = np.zeros((len(reads), W), dtype=np.uint64)
    step = max(1, (1 << 22) // k)
    for s0 in range(0, len(reads), step):
        r, p = reads[s0:s0 + step], poss[s0:s0 + step]
        base = p[:, None] + np.arange(k, dtype=np.int64)[None, :]
        byte = packed[off.astype(np.int64)[r][:, None] + (base >> 2)].astype(np.uint64)
        code = (byte >> (np.uint64(6) - np.uint64(2) * (base & 3).astype(np.uint64))) & np.uint64(3)
        twin = np.uint64(3) - code[:, ::-1]

        def pack(x):
            w = np.zeros((len(x), W), dtype=np.uint64)
            for j in range(W):
                seg = x[:, 32 * j:32 * j + 32]
                sh = np.uint64(62) - np.uint64(2) * np.arange(seg.shape[1], dtype=np.uint64)
                w[:, j] = np.bitwise_or.reduce(seg << sh[None, :], axis=1)
            return w

        f, t = pack(code), pack(twin)
        lt = np.zeros(len(f), dtype=bool)
        eq = np.ones(len(f), dtype=bool)
        for j in range(W):
            lt |= eq & (t[:, j] < f[:, j])
            eq &= t[:, j] == f[:, j]
        out[s0:s0 + step] = np.where(lt[:, None], t, f)
    return out


def _column_words(A):
    return np.stack([A[n] for n in ("kmers", "kmers_lo", "kmers_lo2") if A.get(n) is not None], axis=1)


@pytest.mark.parametrize("k", [63, 95])
def test_host_canonical_words_match_the_oracle(k):
    """The host computation the full-size tests check sampled columns with: at every entry of the oracle's A, the canonical k-mer at (read, pos) is
    its column's, all words."""
    packed, off, lens, _ = elba_amd.synth_reads(500 + k, 40000, 10, 1500, 400, error_rate=0.03, min_len=200)
    o = gu.oracle_run(packed, off, lens, k, 2, 40)
    A = o.A()
    assert A["Z"] > 1000
    col = np.repeat(np.arange(A["N"]), np.diff(A["colptr"].astype(np.int64)))
    got = canonical_words(packed, off, A["csc_read"], A["csc_pos"], k)
    assert (got == _column_words(A)[col]).all()


# ---- inputs ---------------------------------------------------------------------------------------------------------------------------------------

def _parity_seqs(k):
    """the reads of test_two_word_kmers_full_pipeline: the golden small sets and reads of k - 1 ... 129 bases"""
    rng = np.random.default_rng(k)
    seqs = util.read_fasta(os.path.join(G, "small_clean.fa")) + util.read_fasta(os.path.join(G, "small_err.fa"))
    seqs += [bytes(rng.choice(list(b"ACGT"), n).tolist()) for n in (k - 1, k, k + 1, k + 2, k + 3, 64, 65, 96, 97, 127, 128, 129)]
    return seqs


def _synth_seqs(seed, err):
    reads, _ = synth.make_reads(seed, 60000, 10, 2000, 500, error=err, min_len=150)
    return list(reads)


def _run(e):
    ks = e.count_kmers()
    e.create_kmer_matrix()
    st = e.create_seed_matrix()
    return ks, st, e.export_kmer_matrix(), e.export_csr(), e.kmer_histogram()


def _same(a, b):
    """two results of _run: counts, A (all words), B, the histogram and the SpGEMM statistics bit for bit"""
    assert all(a[0][f] == b[0][f] for f in _COUNT_FIELDS)
    assert all(a[1][f] == b[1][f] for f in _SEED_FIELDS)
    gu.assert_A_equal(a[2], b[2])
    for n in ("kmers_lo", "kmers_lo2"):
        assert (a[2][n] is None) == (b[2][n] is None) and (a[2][n] is None or (a[2][n] == b[2][n]).all())
    gu.assert_B_equal(a[3], b[3])
    assert len(a[4]) == len(b[4]) and (a[4] == b[4]).all()


def _engine(packed, off, lens, k, lo, up, cap=0):
    e = elba_amd.Engine(k, lo, up, options={"kmer_batch_instances": cap} if cap else None)
    e.set_reads(packed, off, lens)
    return e


def _unbatched(packed, off, lens, k, lo, up, o):
    e = _engine(packed, off, lens, k, lo, up)
    ref = _run(e)
    assert e.get_stat("kmer_path") == 0 and e.get_stat("kmer_passes") == 1
    assert e.get_stat("kmer_largest_pass") == ref[0]["instances"]
    e.close()
    assert (ref[0]["instances"], ref[0]["distinct"], ref[0]["reliable"], ref[0]["entries"]) == (o.stat("I"), o.stat("ndistinct"), o.stat("N"), o.stat("Z"))
    gu.assert_stats_equal(ref[1], o)
    gu.assert_A_equal(ref[2], o.A())
    gu.assert_B_equal(ref[3], o.B())
    return ref


def _batched(packed, off, lens, k, lo, up, cap, ref, o):
    e = _engine(packed, off, lens, k, lo, up, cap)
    got = _run(e)
    passes, largest = e.get_stat("kmer_passes"), e.get_stat("kmer_largest_pass")
    assert e.get_stat("kmer_path") == 0 and passes >= 2, passes
    assert e.get_stat("kmer_peak_bytes") > 0
    e.close()
    _same(got, ref)
    gu.assert_stats_equal(got[1], o)
    gu.assert_A_equal(got[2], o.A())
    return passes, largest


# ---- 1. forced passes equal the unbatched run and the oracle ------------------------------------------------------------------------------------

@pytest.mark.parametrize("k", [33, 45, 63, 65, 77, 95])
@pytest.mark.parametrize("lo,up", [(2, 12), (2, 40)])
def test_forced_long_passes_equal_the_unbatched_run_and_the_oracle(k, lo, up):
    """The parity reads plus an error-rich synthetic set (5-10 % error), caps I / 2 + 1, I / 7 and I / 64: counts, A (every word, pointers, entries),
    the k-mer histogram, B and the SpGEMM statistics equal the unbatched run's and the oracle's; no pass exceeds the cap (no 24-bit prefix of
    these reads holds that many instances)."""
    seqs = _parity_seqs(k) + _synth_seqs(700 + k + up, 0.05 + 0.01 * (k % 6))
    packed, off, lens = po.pack_reads(seqs)
    o = gu.oracle_run(packed, off, lens, k, lo, up, threads=8)
    ref = _unbatched(packed, off, lens, k, lo, up, o)
    I = int(ref[0]["instances"])
    for cap in (I // 2 + 1, I // 7, I // 64):
        passes, largest = _batched(packed, off, lens, k, lo, up, cap, ref, o)
        assert largest <= cap, (cap, largest)
        assert passes >= (I + cap - 1) // cap


# ---- 2. dominant prefixes ---------------------------------------------------------------------------------------------------------------------------

def _dominant(shape, k):
    base = _synth_seqs(221, 0.05)
    rng = np.random.default_rng(223)
    if shape == "poly_a":
        return base + [b"A" * 600] * 3000, 3000 * (600 - k + 1)       # 1.6 M instances of the k-mer 0 (never kept: more than UPPER copies)
    if shape == "at_rich":
        g = np.where(rng.random(200000) < 0.01, rng.choice(np.frombuffer(b"CG", dtype=np.uint8), 200000),
                     rng.choice(np.frombuffer(b"AT", dtype=np.uint8), 200000)).astype(np.uint8).tobytes()
        return base + [g[s:s + 3000] for s in rng.integers(0, 200000 - 3000, size=200)], 0
    unit = b"ACGGTCATTGCA"                                               # a tandem repeat of a 12-base unit, with a few errors
    reads = []
    for _ in range(400):
        r = bytearray((unit * 150)[int(rng.integers(0, 12)):][:1500])
        for p in rng.integers(0, len(r), size=4):
            r[p] = int(rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8)))
        reads.append(bytes(r))
    return base + reads, 0


@pytest.mark.parametrize("k", [63, 95])
@pytest.mark.parametrize("shape", ["poly_a", "at_rich", "tandem"])
def test_long_passes_hold_a_dominant_prefix(shape, k):
    """Ordinary reads plus poly-A reads (one 24-bit prefix holds most instances: a pass of its own, larger than the cap), AT-rich reads, or a
    tandem repeat of a 12-base unit (a handful of k-mers with huge counts), at small caps: the result is the unbatched run's and the oracle's."""
    lo, up = 2, 12
    seqs, n0 = _dominant(shape, k)
    packed, off, lens = po.pack_reads(seqs)
    o = gu.oracle_run(packed, off, lens, k, lo, up, threads=8)
    ref = _unbatched(packed, off, lens, k, lo, up, o)
    I = int(ref[0]["instances"])
    for cap in (I // 3 + 1, I // 50):
        passes, largest = _batched(packed, off, lens, k, lo, up, cap, ref, o)
        assert largest <= I
        if shape == "poly_a":
            assert n0 > I // 2 and largest >= n0 > cap, (n0, largest, cap)


# ---- 3. empty passes ------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k", [45, 77])
def test_long_passes_with_nothing_to_keep(k):
    """A pass whose k-mers all occur fewer than LOWER times (3000 distinct k-mers behind twelve A: the 24-bit prefix 0, a pass of its own that keeps no
    column), prefix ranges without instances, reads shorter than k and empty reads: the result is the unbatched run's and the oracle's."""
    lo, up = 2, 12
    rng = np.random.default_rng(k)
    singles = [b"A" * 12 + bytes(rng.choice(list(b"CGT"), 1).tolist()) + bytes(rng.choice(list(b"ACGT"), k - 13).tolist()) for _ in range(3000)]
    short = [bytes(rng.choice(list(b"ACGT"), n).tolist()) for n in (1, 5, k - 2, k - 1)] + [b""]
    seqs = short[:2] + _synth_seqs(40 + k, 0.05) + singles + short[2:]
    packed, off, lens = po.pack_reads(seqs)
    o = gu.oracle_run(packed, off, lens, k, lo, up, threads=8)
    ref = _unbatched(packed, off, lens, k, lo, up, o)
    I = int(ref[0]["instances"])
    for cap in (1000, I // 9):
        passes, largest = _batched(packed, off, lens, k, lo, up, cap, ref, o)
        assert largest <= max(cap, 4000)


@pytest.mark.parametrize("k", [33, 95])
def test_long_passes_option_on_zero_instances(k):
    """Every read shorter than k, the option set: nothing is counted, one pass, as without the option."""
    seqs = [b"ACGT" * 5, b"", b"A" * (k - 1)]
    packed, off, lens = po.pack_reads(seqs)
    for cap in (0, 1):
        e = _engine(packed, off, lens, k, 2, 12, cap)
        ks = e.count_kmers()
        assert all(ks[f] == 0 for f in _COUNT_FIELDS)
        assert e.get_stat("kmer_passes") == 1
        e.close()


# ---- 4. state -------------------------------------------------------------------------------------------------------------------------------------

def test_one_engine_counts_with_different_caps_and_new_reads():
    """One engine counts the same reads at two caps and unbatched: A is identical each time; then it takes other reads (fewer, shorter) at a cap
    and its result is theirs alone."""
    k, lo, up = 63, 2, 40
    p1, o1, l1 = po.pack_reads(_parity_seqs(k) + _synth_seqs(81, 0.06))
    p2, o2, l2 = po.pack_reads(_synth_seqs(82, 0.08)[:150])
    or1 = gu.oracle_run(p1, o1, l1, k, lo, up, threads=8)
    or2 = gu.oracle_run(p2, o2, l2, k, lo, up, threads=8)
    ref = _unbatched(p1, o1, l1, k, lo, up, or1)
    I = int(ref[0]["instances"])
    e = _engine(p1, o1, l1, k, lo, up, I // 5)
    got = _run(e)
    assert e.get_stat("kmer_passes") >= 5
    _same(got, ref)
    e.set_option("kmer_batch_instances", I // 2 + 1)
    got = _run(e)
    assert e.get_stat("kmer_passes") >= 2
    _same(got, ref)
    e.set_option("kmer_batch_instances", 0)
    got = _run(e)
    assert e.get_stat("kmer_passes") == 1
    _same(got, ref)
    e.set_reads(p2, o2, l2)
    e.set_option("kmer_batch_instances", 3000)
    got = _run(e)
    assert e.get_stat("kmer_passes") >= 2
    assert (got[0]["instances"], got[0]["distinct"], got[0]["reliable"], got[0]["entries"]) == (or2.stat("I"), or2.stat("ndistinct"), or2.stat("N"), or2.stat("Z"))
    gu.assert_A_equal(got[2], or2.A())
    gu.assert_B_equal(got[3], or2.B())
    gu.assert_stats_equal(got[1], or2)
    e.close()


def _chain(packed, off, lens, k, lo, up, cap):
    e = _engine(packed, off, lens, k, lo, up, cap)
    e.count_kmers()
    passes = e.get_stat("kmer_passes")
    e.create_kmer_matrix()
    st = e.create_seed_matrix()
    al = e.align_seeds()
    ov = e.export_overlaps()
    tr = e.transitive_reduction()
    sg = e.export_string_graph()
    e.close()
    return passes, st, al, ov, tr, sg


def test_batched_k63_matrix_through_alignment_and_transitive_reduction():
    """create_seed_matrix -> align_seeds -> transitive_reduction on an A counted in passes at k = 63 equals the chain on the unbatched A."""
    k, lo, up = 63, 2, 40
    packed, off, lens, _ = elba_amd.synth_reads(91, 300000, 20, 5000, 1200, error_rate=0.01, min_len=1000)
    I = int(np.maximum(lens.astype(np.int64) - (k - 1), 0).sum())
    a = _chain(packed, off, lens, k, lo, up, 0)
    b = _chain(packed, off, lens, k, lo, up, I // 6)
    assert a[0] == 1 and b[0] >= 6
    assert a[1]["nnz"] > 0 and all(a[1][f] == b[1][f] for f in _SEED_FIELDS)
    assert a[2] == b[2] or all(a[2][f] == b[2][f] for f in a[2] if not f.startswith("ms"))
    for x, y in ((a[3], b[3]), (a[5], b[5])):
        assert x["n"] == y["n"] and (x["rows"] == y["rows"]).all() and (x["cols"] == y["cols"]).all() and (x["vals"] == y["vals"]).all()
    assert a[5]["n"] > 0
    assert {f: v for f, v in a[4].items() if not f.startswith("ms")} == {f: v for f, v in b[4].items() if not f.startswith("ms")}


# ---- 5. full size, no option set --------------------------------------------------------------------------------------------------------------------

class _DevArray:
    """A device pointer of the library as something torch can wrap without a copy (__cuda_array_interface__)."""

    def __init__(self, ptr, n, typestr):
        self.__cuda_array_interface__ = {"shape": (int(n),), "typestr": typestr, "data": (int(ptr), False), "version": 2}


def _digest(t):
    """an order-sensitive digest of a device array (int64 arithmetic wraps): two sums over chunks, weighted by place and mixed"""
    import torch
    a = b = 0
    n = t.numel()
    step = 1 << 27
    for s0 in range(0, n, step):
        x = t[s0:s0 + step].to(torch.int64)
        w = torch.arange(s0, s0 + x.numel(), device=x.device, dtype=torch.int64) * 2 + 1
        a = (a + int((x * w).sum().item())) & 0xFFFFFFFFFFFFFFFF
        b = (b + int((x ^ (x >> 29) ^ (w << 17)).sum().item())) & 0xFFFFFFFFFFFFFFFF
    return a, b


def _views(e):
    import torch
    v = e.device_view()
    t = lambda ptr, n, ts: torch.as_tensor(_DevArray(ptr, n, ts), device="cuda")      # noqa: E731
    return v, t(v["a_kmers"], v["N"], "<i8"), t(v["a_colptr"], v["N"] + 1, "<i4"), t(v["a_csc"], v["Z"], "<i8")


def _A_digests(e):
    v, tk, tcp, tcsc = _views(e)
    return dict(N=v["N"], Z=v["Z"], kmers=_digest(tk), colptr=_digest(tcp), csc=_digest(tcsc))


def _check_sampled_columns(e, packed, off, k, lo, up, nsample=1000):
    """every entry of nsample random columns: the canonical k-mer at (read, pos), all words, is the same for the whole column and its first word is
    the column's"""
    v, tk, tcp, tcsc = _views(e)
    rng = np.random.default_rng(k)
    cols = np.sort(rng.choice(int(v["N"]), size=nsample, replace=False))
    ptr = tcp.cpu().numpy().astype(np.int64) & 0xFFFFFFFF
    kms = tk[torch_index(cols)].cpu().numpy().view(np.uint64)
    reads, poss, which = [], [], []
    for i, j in enumerate(cols):
        ent = tcsc[int(ptr[j]):int(ptr[j + 1])].cpu().numpy().view(np.uint64)
        assert lo <= len(ent) <= up
        reads.append((ent >> np.uint64(32)).astype(np.int64))
        poss.append((ent & np.uint64(0xFFFFFFFF)).astype(np.int64))
        which.append(np.full(len(ent), i))
    reads, poss, which = np.concatenate(reads), np.concatenate(poss), np.concatenate(which)
    w = canonical_words(packed, off, reads, poss, k)
    assert (w[:, 0] == kms[which]).all()
    first = np.searchsorted(which, np.arange(nsample))
    assert (w == w[first][which]).all()
    return len(reads)


def torch_index(a):
    import torch
    return torch.as_tensor(np.asarray(a, dtype=np.int64), device="cuda")


@pytest.mark.parametrize("k,lo,up", [(63, 15, 30), (95, 12, 25)])
def test_more_than_2_32_instances_with_long_kmers_full_size(k, lo, up):
    """hifi reads of a 120 Mb genome at 40x (15 kb, 0.5 % error): ~4.8 G instances of k = 63 / 95, no option set.  The call succeeds in value-range
    passes (before: ELBA_ERR_UNSUPPORTED); the size-independent identities hold; every entry of 1000 sampled columns names its column's k-mer; a
    smaller cap gives the bit-identical A."""
    import torch
    packed, off, lens, info = elba_amd.synth_reads(3, 120_000_000, 40.0, 15000.0, 2000.0, error_rate=0.005, min_len=1000)
    I_expected = int(np.maximum(lens.astype(np.int64) - (k - 1), 0).sum())
    assert I_expected > (1 << 32), I_expected
    free0, total = torch.cuda.mem_get_info()
    e = elba_amd.Engine(k, lo, up)
    e.set_reads(packed, off, lens)
    t0 = time.perf_counter()
    ks = e.count_kmers()
    t_stage = time.perf_counter() - t0
    passes, largest, peak = e.get_stat("kmer_passes"), e.get_stat("kmer_largest_pass"), e.get_stat("kmer_peak_bytes")
    free1, _ = torch.cuda.mem_get_info()
    ms = e.create_kmer_matrix()
    print("full size k=%d: nnz(A)=%d after %d passes" % (k, ks["entries"], passes), flush=True)
    e.release_workspace()          # (the CSR build's sort buffers: the multiplication of a matrix this size needs the room)
    st = e.create_seed_matrix()
    print("full size k=%d L=%d U=%d: instances=%d reliable=%d nnz(A)=%d passes=%d largest_pass=%d stage_ms=%.1f (count %.1f, runs %.1f; wall %.2f s) "
          "peak_gb=%.1f resident_after_count_gb=%.1f free_at_start_gb=%.1f products=%d overlap_nnz=%d"
          % (k, lo, up, ks["instances"], ks["reliable"], ks["entries"], passes, largest, ks["ms_total"], ks["ms_count"], ks["ms_sort"], t_stage,
             peak / 1e9, (free0 - free1) / 1e9, free0 / 1e9, st["products"], st["nnz"]))
    assert e.get_stat("kmer_path") == 0 and passes >= 2
    assert ks["instances"] == I_expected and 0 < ks["entries"] < (1 << 32)
    h = e.kmer_histogram(up + 2)
    c = np.arange(len(h), dtype=np.int64)
    assert int(h.sum()) == ks["reliable"] == ms["ncols"]
    assert int((h * c).sum()) == ks["entries"] == ms["nnz"]
    assert int((h * c * c).sum()) == st["products"]
    assert st["nnz"] == st["nnz_diag"] + 2 * st["nnz_upper"]
    checked = _check_sampled_columns(e, packed, off, k, lo, up)
    assert checked >= 1000 * lo
    ref = _A_digests(e)
    cap = ks["instances"] // 5
    e.set_option("kmer_batch_instances", cap)
    ks2 = e.count_kmers()
    e.create_kmer_matrix()
    assert e.get_stat("kmer_passes") >= 5 and e.get_stat("kmer_largest_pass") <= cap
    assert all(ks2[f] == ks[f] for f in _COUNT_FIELDS)
    assert _A_digests(e) == ref
    print("full size k=%d, cap I/5: passes=%d largest_pass=%d stage_ms=%.1f peak_gb=%.1f"
          % (k, e.get_stat("kmer_passes"), e.get_stat("kmer_largest_pass"), ks2["ms_total"], e.get_stat("kmer_peak_bytes") / 1e9))
    e.close()


def test_celegans_hifi_shape_at_k63():
    """BASELINE configs[3]'s reads (100 Mb at 40x, 15 kb, 0.5 % error) at k = 63: ~3.98 G instances, below 2^32 but beyond what one pass's
    workspace fits in, no option set: counted in passes; the identities hold."""
    import torch
    k, lo, up = 63, 2, 4
    packed, off, lens, info = elba_amd.synth_reads(3, 100_000_000, 40.0, 15000.0, 2000.0, error_rate=0.005, min_len=1000)
    free0, _ = torch.cuda.mem_get_info()
    e = elba_amd.Engine(k, lo, up)
    e.set_reads(packed, off, lens)
    ks = e.count_kmers()
    ms = e.create_kmer_matrix()
    passes = e.get_stat("kmer_passes")
    print("configs[3] shape k=63: instances=%d reliable=%d nnz(A)=%d passes=%d largest_pass=%d stage_ms=%.1f peak_gb=%.1f free_at_start_gb=%.1f"
          % (ks["instances"], ks["reliable"], ks["entries"], passes, e.get_stat("kmer_largest_pass"), ks["ms_total"],
             e.get_stat("kmer_peak_bytes") / 1e9, free0 / 1e9))
    assert ks["instances"] == int(np.maximum(lens.astype(np.int64) - (k - 1), 0).sum()) < (1 << 32)
    assert passes >= 2
    h = e.kmer_histogram(up + 2)
    c = np.arange(len(h), dtype=np.int64)
    assert int(h.sum()) == ks["reliable"] == ms["ncols"] and int((h * c).sum()) == ks["entries"] == ms["nnz"]
    e.close()
