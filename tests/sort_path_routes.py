"""The cases of tests/test_gpu_sort_path_routes.py and of its recorder (tests/golden/record_sort_path_routes.py): small seeded read sets that the
k-mer stage counts by SORTING (csrc/kmer.hip: stage_count_kmers' one-word and multi-word sorts, count_long_kmers_in_passes, stage_dist_count_records),
one per route through that path's host driver.  run_case() returns what the fixture holds of a case: the route (the diagnostic counters), the counts
and SHA-256 digests of the column pointers, the columns, the reliable k-mers (all words) and their counts.  Not recorded: "kmer_peak_bytes" (measured
free memory) and every ms_* time."""
import hashlib

import numpy as np
import torch

import elba_amd
import kmer_stage_routes as msd_routes
import synth
from elba_amd import distributed
from oracle import pyoracle as po

COUNT_STATS = ("kmer_path", "kmer_passes", "kmer_largest_pass")
MATRIX_STATS = ("matrix_csr_words",)
COUNTS = ("instances", "distinct", "reliable", "entries")
LEFT_OUT = ("kmer_peak_bytes", "ms_total", "ms_count", "ms_sort", "ms_lookup")


def _long_base():
    return list(synth.make_reads(221, 60000, 10, 2000, 500, error=0.05, min_len=150)[0])


def _poly_a():
    # one 24-bit prefix (the k-mer 0) holds most instances: a unit above every cap, a pass of its own
    return _long_base() + [b"A" * 600] * 3000


def _at_rich():
    # AT-rich reads: 12-bit bins above the cap whose instances spread over many 24-bit prefixes
    rng = np.random.default_rng(223)
    g = np.where(rng.random(200000) < 0.01, rng.choice(np.frombuffer(b"CG", dtype=np.uint8), 200000),
                 rng.choice(np.frombuffer(b"AT", dtype=np.uint8), 200000)).astype(np.uint8).tobytes()
    return _long_base() + [g[s:s + 3000] for s in rng.integers(0, 200000 - 3000, size=200)]


READS = {
    "poly_a": _poly_a,
    "at_rich": _at_rich,
    "short": lambda: [b"ACGT" * 5, b"", b"A" * 32],
}
_sets = {}


def read_set(name):
    if name in msd_routes.READS:
        return msd_routes.read_set(name)
    if name not in _sets:
        _sets[name] = po.pack_reads(READS[name]())
    return _sets[name]


def instances(name, k):
    return int(np.maximum(read_set(name)[2].astype(np.int64) - (k - 1), 0).sum())


NO_MSD = {"kmer_no_msd": 1}
# name -> (reads, k, lower, upper, options, a cap of kmer_batch_instances as a divisor of the instances or None)
CASES = {
    # one-word k-mers the partition declines
    "k17_packed_fused": ("r17", 17, 2, 8, NO_MSD, None),
    "k17_emit_plain": ("r17", 17, 2, 8, dict(NO_MSD, emit_plain=1), None),
    "k17_unfused": ("r17", 17, 2, 8, dict(NO_MSD, kmer_unfused=1), None),
    "k17_upper80": ("r17", 17, 2, 80, NO_MSD, None),
    "k17_pairs": ("r17", 17, 2, 8, dict(NO_MSD, kmer_pairs=1), None),
    "k31_pairs_by_width": ("r31", 31, 2, 8, NO_MSD, None),
    "k17_drop1": ("r17", 17, 2, 12, dict(NO_MSD, kmer_drop=1), None),
    "k17_drop3": ("r17", 17, 2, 12, dict(NO_MSD, kmer_drop=3), None),
    "k17_nothing_kept": ("r31", 17, 50, 60, NO_MSD, None),
    # two and three words
    "k33": ("r17", 33, 2, 8, {}, None),
    "k63": ("r17", 63, 2, 8, {}, None),
    "k65": ("r17", 65, 2, 8, {}, None),
    "k95": ("r17", 95, 2, 8, {}, None),
    "k33_passes": ("r17", 33, 2, 8, {}, 3),
    "k65_passes": ("r17", 65, 2, 8, {}, 3),
    "k63_unit_above_cap": ("poly_a", 63, 2, 12, {}, 6),
    "k95_heavy_bin_refined": ("at_rich", 95, 2, 12, {}, 200),
    "k33_nothing_kept": ("r31", 33, 50, 60, {}, None),
    "k33_passes_nothing_kept": ("r31", 33, 50, 60, {}, 3),
}
PASSES_FORCED = tuple(n for n, c in CASES.items() if c[5])
ZERO_CASE = "k33_zero_instances_cap_set"
ENGINE_CASE = "one_engine_two_counts"
TWICE_CASE = "matrix_twice_after_one_count"
DIST_CASES = {"dist_owner_k17": 17, "dist_owner_k33": 33, "dist_owner_k65": 65}
ALL_CASES = tuple(CASES) + (ZERO_CASE, ENGINE_CASE, TWICE_CASE) + tuple(DIST_CASES)


def _sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def _matrix(e):
    e.create_kmer_matrix()
    A = e.export_kmer_matrix()
    words = [A[n] for n in ("kmers", "kmers_lo", "kmers_lo2") if A[n] is not None]
    rec = {s: int(e.get_stat(s)) for s in MATRIX_STATS}
    rec.update(colptr=_sha(A["colptr"]), csc_read=_sha(A["csc_read"]), csc_pos=_sha(A["csc_pos"]), kmer_words=len(words),
               kmers=_sha(np.stack(words, axis=1)), counts=_sha(np.diff(A["colptr"])), kmer_histogram=_sha(e.kmer_histogram().astype(np.int64)))
    return rec, A


def _count(e, check):
    ks = e.count_kmers()
    rec = {s: int(e.get_stat(s)) for s in COUNT_STATS}
    rec.update({f: int(ks[f]) for f in COUNTS})
    m, A = _matrix(e)
    rec.update(m)
    if check:
        check(ks, A)
    return rec


def options(name):
    reads, k, lo, up, opts, div = CASES[name]
    opts = dict(opts)
    if div:
        opts["kmer_batch_instances"] = instances(reads, k) // div + 1
    return opts


def _dist(name):
    """The owner side of exchange #1 on one rank: the rank's own records (made on the device, brought into one fixed shuffled order on the host: they
    arrive in no particular order), counted by elba_dist_count_records; the owner's reliable k-mers and its columns as the panel it would send."""
    from dist_sim import NumpyBackend
    k, lo, up = DIST_CASES[name], 2, 8
    kw = distributed.kmer_words(k)
    packed, off, lens = read_set("r17")
    be = distributed.HipBackend(k, lo, up, 0)
    be.set_reads(packed, off, lens, 0)
    n = int(be.count_owners(1)[0])
    send = be.empty_records(n, kw + 1)
    be.fill_send(1, send, np.zeros(1, dtype=np.int64))
    be.synchronize()
    host = send.cpu().numpy().view(np.uint64)
    host = host[np.lexsort([host[:, w] for w in range(kw, -1, -1)])]
    host = np.ascontiguousarray(host[np.random.default_rng(9).permutation(n)])
    rec = torch.from_numpy(host.view(np.int64)).to(be.dev)
    st = be.count_records(rec)
    N = int(st["reliable"])
    rel = be.reliable_kmers(N).cpu().numpy().view(np.uint64).reshape(-1, kw)
    be.set_kmer_id_base(0, N)
    bounds = np.array([0, len(lens)], dtype=np.int64)
    pc = be.panel_counts(1, bounds)
    panel = be.empty_records(int(pc[0]), 2)
    be.panel_fill(1, bounds, panel, np.zeros(1, dtype=np.int64))
    be.synchronize()
    cols = panel.cpu().numpy().view(np.uint64)
    cols = cols[np.lexsort((cols[:, 1], cols[:, 0]))]
    del rec
    be.e.close()
    # the same records through the numpy stand-in
    nb = NumpyBackend(k, lo, up)
    want = nb.count_records(torch.from_numpy(host.view(np.int64)))
    assert tuple(int(st[f]) for f in COUNTS) == tuple(int(want[f]) for f in COUNTS)
    assert np.array_equal(rel, np.asarray(nb.rel).reshape(-1, kw))
    assert np.array_equal(cols[:, 1], np.concatenate(nb.cols + [np.zeros(0, np.uint64)]))
    assert np.array_equal(cols[:, 0], np.repeat(np.arange(N, dtype=np.uint64), [len(c) for c in nb.cols]))
    out = {f: int(st[f]) for f in COUNTS}
    out.update(records=_sha(host), own_kmers=_sha(rel), own_columns=_sha(cols))
    return out


def run_case(name, check=None):
    """The record of one case (a list of two for ENGINE_CASE and TWICE_CASE).  check(counts, A, reads, k, lower, upper), if given, is called with every
    count's statistics and exported matrix."""
    def chk(reads, k, lo, up):
        return check and (lambda ks, A: check(ks, A, reads, k, lo, up))
    if name in DIST_CASES:
        return _dist(name)
    if name == ZERO_CASE:
        # every read shorter than k, the cap set: nothing is counted (no matrix is built of nothing)
        e = elba_amd.Engine(33, 2, 12, options={"kmer_batch_instances": 1})
        e.set_reads(*read_set("short"))
        ks = e.count_kmers()
        rec = {s: int(e.get_stat(s)) for s in COUNT_STATS}
        rec.update({f: int(ks[f]) for f in COUNTS})
        e.close()
        return rec
    if name == ENGINE_CASE:
        # two counts in a row on one engine: few reads in two passes, then more reads in four — every buffer of the path is regrown in between
        e = elba_amd.Engine(33, 2, 8, options={"kmer_batch_instances": instances("r17_few", 33) // 2 + 1})
        e.set_reads(*read_set("r17_few"))
        first = _count(e, chk("r17_few", 33, 2, 8))
        e.set_reads(*read_set("r17"))
        e.set_option("kmer_batch_instances", instances("r17", 33) // 4 + 1)
        second = _count(e, chk("r17", 33, 2, 8))
        e.close()
        return [first, second]
    reads, k, lo, up, _, _ = CASES["k17_packed_fused" if name == TWICE_CASE else name]
    e = elba_amd.Engine(k, lo, up, options=options("k17_packed_fused" if name == TWICE_CASE else name))
    e.set_reads(*read_set(reads))
    rec = _count(e, chk(reads, k, lo, up))
    if name == TWICE_CASE:
        # the CSR build consumed the sort keys the fused column pass left: a second build expands the column pointers instead
        again, A = _matrix(e)
        if check:
            check(None, A, reads, k, lo, up)
        rec = [rec, again]
    e.close()
    return rec
