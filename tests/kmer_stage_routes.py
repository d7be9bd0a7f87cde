"""The cases of tests/test_gpu_kmer_stage_routes.py and of its recorder (tests/golden/record_kmer_stage_routes.py): small seeded read sets on which
"kmer_msd" forces the two-level partition, one per route through the k-mer stage's host driver (csrc/kmer_msd.hip, msd_run).  run_case() returns what
the fixture holds of a case: the route (the diagnostic counters), the counts and SHA-256 digests of what does not depend on workgroup scheduling — the
column pointers, the columns, the reliable k-mers and their counts (not the padded column store, the slot count under gather slots or the sort words)."""
import functools
import hashlib

import numpy as np

import elba_amd
import gpu_util as gu
import synth
from oracle import pyoracle as po

_BASES = np.frombuffer(b"ACGT", dtype=np.uint8)
ROUTE_STATS = ("kmer_path", "kmer_passes", "kmer_buckets", "kmer_crowded_buckets", "kmer_crowded_small", "kmer_largest_pass")
COUNTS = ("instances", "distinct", "reliable", "entries")


def _random_seqs(rng, n, length):
    return [t.tobytes() for t in _BASES[rng.integers(0, 4, size=(n, length))]]


def _satellite(rng, lead, tail_len, trail, n_single, n_rep):
    """31-mers of one leading run: n_single of them once, n_rep of them 2-4 times (the reliable ones: LOWER = 2, UPPER = 8)."""
    kms = [lead + t + trail for t in _random_seqs(rng, n_single + n_rep, tail_len)]
    reps = rng.integers(2, 5, size=n_rep)
    return kms[:n_single] + [s for s, c in zip(kms[n_single:], reps) for _ in range(int(c))]


def _shuffled(seqs, seed):
    seqs = list(seqs)
    np.random.default_rng(seed).shuffle(seqs)
    return seqs


def _reads17():
    reads, _ = synth.make_reads(501, 60000, 10, 400, 100, error=0.05, min_len=100)
    # low-complexity reads: runs of one canonical k-mer at neighbouring positions, k-mers far beyond UPPER
    return _shuffled(list(reads) + [b"A" * 300, b"AC" * 200, b"T" * 150 + b"G" * 150, b"ACG" * 120, b"ACGT" * 90] * 3, 5)


def _reads17_dense_bucket():
    # 30 k-mers that share their leading nine bases (one bucket of the 2 x 9 partitioned bits), four copies each: a bucket of 120 kept entries
    rng = np.random.default_rng(505)
    return _shuffled(_reads17() + [b"A" * 8 + b"C" + t for t in _random_seqs(rng, 30, 8)] * 4, 8)


def _reads17_poly_a():
    reads, _ = synth.make_reads(502, 60000, 10, 400, 100, error=0.05, min_len=100)
    return _shuffled(list(reads) + [b"A" * 1016] * 800, 6)      # 800 000 instances of the k-mer 0: one first digit holds more than half of the input


def _reads31(where, n_rep):
    reads, _ = synth.make_reads(503, 60000, 10, 400, 100, error=0.10, min_len=100)
    lead, tail_len, trail = {"first": (b"A" * 10, 21, b""), "middle": (b"C" + b"A" * 9, 19, b"GG")}[where]
    return _shuffled(list(reads) + _satellite(np.random.default_rng(504 + n_rep), lead, tail_len, trail, 3500, n_rep), 7)


READS = {
    "r17": _reads17,
    "r17_dense_bucket": _reads17_dense_bucket,
    "r17_poly_a": _reads17_poly_a,
    "r17_few": lambda: _reads17()[:300],
    "r31": lambda: list(synth.make_reads(503, 60000, 10, 400, 100, error=0.10, min_len=100)[0]),
    "r31_sat_first": lambda: _reads31("first", 1000),
    "r31_sat_middle": lambda: _reads31("middle", 300),
}


@functools.lru_cache(maxsize=None)
def read_set(name):
    return po.pack_reads(READS[name]())


def instances(name, k):
    return int(np.maximum(read_set(name)[2].astype(np.int64) - (k - 1), 0).sum())


# name -> (reads, k, lower, upper, options, a cap of kmer_batch_instances as a divisor of the instances or None)
CASES = {
    "k17_plain": ("r17", 17, 2, 8, {}, None),
    "k17_no_rank": ("r17", 17, 2, 8, {"msd_no_rank": 1}, None),
    "k17_rank": ("r17", 17, 2, 8, {"msd_rank": 1}, None),
    "k17_small_cap": ("r17_dense_bucket", 17, 2, 8, {"msd_small_cap": 64}, None),
    "k17_batched": ("r17", 17, 2, 8, {}, 3),
    "k17_batched_dominant_digit": ("r17_poly_a", 17, 2, 8, {}, 3),
    "k31_plain": ("r31", 31, 2, 8, {}, None),
    "k31_crowded": ("r31_sat_first", 31, 2, 8, {"msd_wide_bits": 12}, None),
    "k31_batched_crowded": ("r31_sat_first", 31, 2, 8, {}, 3),
    "k31_batched_crowded_small_parent": ("r31_sat_middle", 31, 2, 8, {}, 3),
    "slot_cap_one_pass": ("r17", 17, 2, 8, {"ell_slot_cap": 100}, None),
    "slot_cap_batched": ("r17", 17, 2, 8, {"ell_slot_cap": 100}, 3),
    "measure_prep": ("r17", 17, 2, 8, {"measure_prep": 1}, None),
}
TRIPLES_CASES = ("triples", "triples_empty_column")
ENGINE_CASE = "one_engine_two_routes"
ALL_CASES = tuple(CASES) + TRIPLES_CASES + (ENGINE_CASE,)


def _sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def _digests(e, with_kmers=True):
    v = e.device_view()
    colptr = gu.host_copy(v["a_colptr"], v["N"] + 1, np.uint32)
    out = {"a_colptr": _sha(colptr), "a_csc": _sha(gu.host_copy(v["a_csc"], v["Z"], np.uint64)), "rel_counts": _sha(np.diff(colptr.astype(np.int64)))}
    if with_kmers:
        out["rel_kmers"] = _sha(gu.host_copy(v["a_kmers"], v["N"], np.uint64))
        out["kmer_histogram"] = _sha(e.kmer_histogram().astype(np.int64))
    return out


def _count(e, check):
    ks = e.count_kmers()
    rec = {s: int(e.get_stat(s)) for s in ROUTE_STATS}
    rec.update({f: int(ks[f]) for f in COUNTS})
    e.create_kmer_matrix()
    rec.update(_digests(e))
    if check:
        check(e, ks)
    return rec


def _options(name):
    reads, k, lo, up, opts, div = CASES[name]
    opts = dict(opts, kmer_msd=1)
    if div:
        opts["kmer_batch_instances"] = instances(reads, k) // div + 1
    return opts


def _triples(name):
    """A of the k = 17 reads, built on the device and handed back as shuffled device triples to an engine with "kmer_msd"; the second case without
    the entries of one column (the column stays: empty)."""
    import torch
    packed, off, lens = read_set("r17")
    e, ks, ms, st = gu.gpu_full(packed, off, lens, 17, 2, 8)
    Z, M, N = int(ms["nnz"]), int(ms["nrows"]), int(ms["ncols"])
    dr = torch.empty(Z, dtype=torch.int64, device="cuda"); dc = torch.empty(Z, dtype=torch.int64, device="cuda"); dv = torch.empty(Z, dtype=torch.int32, device="cuda")
    e.export_triples_device(dr.data_ptr(), dc.data_ptr(), dv.data_ptr())
    perm = torch.from_numpy(np.random.default_rng(5).permutation(Z)).to("cuda")
    dr, dc, dv = dr[perm].contiguous(), dc[perm].contiguous(), dv[perm].contiguous()
    if name == "triples_empty_column":
        keep = dc != int(dc[0])
        dr, dc, dv = dr[keep].contiguous(), dc[keep].contiguous(), dv[keep].contiguous()
    e2 = elba_amd.Engine(17, 2, 8, options={"kmer_msd": 1})
    m2 = e2.set_kmer_matrix_device(M, N, int(dr.numel()), dr.data_ptr(), dc.data_ptr(), dv.data_ptr())
    rec = {"triples_path": int(e2.get_stat("triples_path")), "ncols": int(m2["ncols"]), "nnz": int(m2["nnz"])}
    rec.update(_digests(e2, with_kmers=False))
    e.close(); e2.close()
    return rec


def run_case(name, check=None):
    """The record of one case (a list of two for ENGINE_CASE).  check(engine, counts, reads, k, lower, upper), if given, is called on every counted engine."""
    if name in TRIPLES_CASES:
        return _triples(name)
    if name == ENGINE_CASE:
        # two counts in a row on one engine: few reads in two passes, then more reads in four — every buffer of the stage is regrown in between
        e = elba_amd.Engine(17, 2, 8, options={"kmer_msd": 1, "kmer_batch_instances": instances("r17_few", 17) // 2 + 1})
        e.set_reads(*read_set("r17_few"))
        first = _count(e, check and (lambda eng, ks: check(eng, ks, "r17_few", 17, 2, 8)))
        e.set_reads(*read_set("r17"))
        e.set_option("kmer_batch_instances", instances("r17", 17) // 4 + 1)
        second = _count(e, check and (lambda eng, ks: check(eng, ks, "r17", 17, 2, 8)))
        e.close()
        return [first, second]
    reads, k, lo, up, _, _ = CASES[name]
    e = elba_amd.Engine(k, lo, up, options=_options(name))
    e.set_reads(*read_set(reads))
    rec = _count(e, check and (lambda eng, ks: check(eng, ks, reads, k, lo, up)))
    if "measure_prep" in CASES[name][4]:
        rec["prep_measured"] = int(e.get_stat("spgemm_prep_us") >= 0 and e.get_stat("emit_us") > 0)      # (the emit ran twice, between its timers)
    e.close()
    return rec

