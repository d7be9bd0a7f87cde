"""The cases of tests/test_gpu_overlap_routes.py and of its recorder (tests/golden/record_overlap_routes.py): small matrices, one per route through the
host driver of the overlap SpGEMM (csrc/spgemm.hip: the plan of csrc/ov_plan.hpp, the tier table, the steps over OvRun, the sharded entry points).
run_case() returns what the fixture holds of a case — per call SHA-256 digests of B and the statistics that do not depend on workgroup scheduling — and
checks every call's B against the oracle and the rows the tiers completed against the non-empty rows of A."""
import functools
import hashlib

import numpy as np

import dist_sim
import elba_amd
import gpu_util as gu
from elba_amd.distributed import DistributedOverlap, HipBackend, partition_by_bases
from oracle import pyoracle as po

PINNED_STATS = ("nnz", "nnz_before_prune", "nnz_diag", "nnz_upper", "max_numshared", "products", "passes")


def _concat(sets):
    packed, off, lens, base = [], [], [], 0
    for (p, o, l, _) in sets:
        nb = int(o[-1]) + (int(l[-1]) + 3) // 4 if len(l) else 0
        packed.append(p[:nb]); off.append(o + np.uint64(base)); lens.append(l); base += nb
    return np.concatenate(packed + [np.zeros(16, np.uint8)]), np.concatenate(off), np.concatenate(lens)


def _long_positions():
    long_ = elba_amd.synth_reads(53, 90000, 6, 70000, 4000, error_rate=0.05, min_len=66000)
    short = elba_amd.synth_reads(54, 90000, 6, 3000, 500, error_rate=0.05, min_len=500)
    return _concat([short, long_])


# name -> (the reads, k, lower, upper)
READS = {
    # 15 %-error reads (tests/test_gpu_spgemm_spec.py's "small"): mostly two-read columns, Z < 3 N — one gather trip, the reads-path instantiation
    "reads15": (lambda: elba_amd.synth_reads(7, 200_000, 30.0, 3000.0, 500.0, error_rate=0.15, min_len=1000)[:3], 17, 2, 8),
    # 10 %-error reads: Z >= 3 N — two gather trips ("dk" = 1 chosen), the general kernel whatever the options
    "reads": (lambda: elba_amd.synth_reads(61, 200000, 16, 3000, 900, error_rate=0.10, min_len=200)[:3], 17, 2, 8),
    "sampled": (lambda: elba_amd.synth_reads(72, 320000, 24, 800, 250, error_rate=0.06, min_len=120)[:3], 17, 2, 12),
    "dense": (lambda: elba_amd.synth_reads(91, 60000, 30, 3000, 600, error_rate=0.01, min_len=500, repeat_families=3, repeat_fraction=0.1, repeat_len=400)[:3], 17, 2, 40),
    "long": (_long_positions, 17, 2, 30),
    "repeat": (lambda: elba_amd.synth_reads(8, 60000, 15, 2500, 400, error_rate=0.05)[:3], 17, 2, 12),
    "wide": (lambda: elba_amd.synth_reads(6, 200, 2200, 100, 0, error_rate=0.0, min_len=100)[:3], 21, 2, 20000),
    "sharded": (lambda: elba_amd.synth_reads(36, 250000, 15, 4000, 900, error_rate=0.10, min_len=200)[:3], 17, 2, 8),
}


@functools.lru_cache(maxsize=None)
def read_set(name):
    return READS[name][0]()


def _scan_triples():
    """140 000 rows (M + 1 > 2^17: the row pointers of B come from k_sum_counts + the scan), a few thousand entries among 600 of them."""
    rng = np.random.default_rng(140)
    M, ncol = 140000, 1500
    hot = rng.choice(M, 600, replace=False)
    rows, cols, vals = [], [], []
    for c in range(ncol):
        r = np.unique(rng.choice(hot, int(rng.integers(2, 6))))
        rows.append(r); cols.append(np.full(len(r), c)); vals.append(rng.integers(0, 4000, len(r)))
    return M, ncol, np.concatenate(rows), np.concatenate(cols), np.concatenate(vals).astype(np.uint32)


def _one_row_triples():
    return 1, 3, np.zeros(3, np.int64), np.arange(3), np.array([5, 9, 14], dtype=np.uint32)


def _empty_triples():
    return 4, 2, np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros(0, np.uint32)


TRIPLES = {"escalation": gu.escalation_triples, "scan": _scan_triples, "one_row": _one_row_triples, "empty": _empty_triples}

# one engine, calls in a row.  name -> (matrix, engine options, engine keywords, the calls: each a dict of options set before it, expected overlap_spec or None)
_READS_OFF = [{"ov_generic": 1}, {"no_symmetry": 1}, {"no_pay": 1}, {"tune3": 1}, {"mir32": 1}, {"no_ell": 1}, {"no_hints": 1}, {"no_inline": 1}, {"no_sample": 1}, {"no_slab": 1},
              {"dk": 0}, {"dk": 1}, {"dk": 2}, {"dk": 4}, {"tune4": 1}, {"tune4": 2}, {"tune7": 3}, {"tune7": 6}, {"tune5": 6}]
ENGINE_CASES = {
    "reads_whole": ("reads", {}, {}, [{}, {}, {"overlap_cold_calls": 1}], 0),
    "reads15_whole": ("reads15", {}, {}, [{}, {}, {"overlap_cold_calls": 1}], 1),
    "sampled_slabs": ("sampled", {}, {}, [{}, {}, {"slab_q16": 1}, {"slab_q16": 1 << 18}], None),
    "dense": ("dense", {}, {}, [{}, {}], 0),
    "dense_no_suffix": ("dense", {"no_suffix": 1}, {}, [{}, {}], 0),
    "dense_no_row_order": ("dense", {"no_row_order": 1}, {}, [{}, {}], 0),
    "dense_up0": ("dense", {"dense_up": 0}, {}, [{}, {}], 0),
    "dense_up2": ("dense", {"dense_up": 2}, {}, [{}, {}], 0),
    "records_32_bytes": ("long", {}, {}, [{}, {}], 0),
    "escalation_hbm": ("escalation", {}, {}, [{}], 0),      # (196 M entries of B: one call)
    "repeated_pass": ("repeat", {}, {"workspace_hint_bytes": 2400}, [{}, {}], None),
    "wide_rows": ("wide", {}, {}, [{}, {}], None),
    "row_pointers_by_scan": ("scan", {}, {}, [{}, {}], None),
    "empty_matrix": ("empty", {}, {}, [{}, {}], None),
    "one_row": ("one_row", {}, {}, [{}, {}], None),
}
for _o in _READS_OFF:      # ("no_sample" and "no_slab" are not among the switches the reads-path instantiation fixes: they keep it)
    _n = "_".join("%s_%d" % kv for kv in _o.items())
    ENGINE_CASES["reads_" + _n] = ("reads", _o, {}, [{}, {}], 0)
    ENGINE_CASES["reads15_" + _n] = ("reads15", _o, {}, [{}, {}], 1 if set(_o) & {"no_sample", "no_slab"} else 0)
SLAB_Q16_PINNED = {"sampled_slabs": (1, 2, 3)}      # the calls whose slab ratio is carried over or forced

# sharded: name -> (world, bounds or None (partition_by_bases), row blocks, exchange)
SHARDED_CASES = {}
for _w in (2, 3):
    for _x in (True, "tiny", "counted", False):
        SHARDED_CASES["sharded_w%d_%s" % (_w, {True: "slots", False: "no_exchange"}.get(_x, _x))] = (_w, None, 1, _x)
SHARDED_CASES["sharded_empty_rank"] = (3, "empty_middle", 1, True)
SHARDED_CASES["sharded_empty_rank_counted"] = (3, "empty_middle", 1, "counted")
SHARDED_CASES["one_engine_two_row_blocks"] = (1, None, 2, False)
ALL_CASES = tuple(ENGINE_CASES) + tuple(SHARDED_CASES)


def _sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def _record(B, st, spec, slab_q16=None):
    rec = {"b_rowptr": _sha(B["rowptr"].astype(np.int64)), "b_col": _sha(B["col"].astype(np.int64)), "b_val": _sha(B["val"])}
    rec.update({f: int(st[f]) for f in PINNED_STATS})
    rec["overlap_spec"] = int(spec)
    if slab_q16 is not None:
        rec["overlap_slab_q16"] = int(slab_q16)
    return rec


@functools.lru_cache(maxsize=None)
def oracle(matrix):
    """(the oracle's B, the number of non-empty rows of A) of a read set or a triples matrix; computed once, shared, never changed"""
    if matrix in TRIPLES:
        M, ncol, rows, cols, vals = TRIPLES[matrix]()
        o = po.Oracle(17, 2, 8)
        o.set_triples(M, ncol, rows, cols, vals)
        o.spgemm(8)
        return o.B(), len(np.unique(rows))
    _, k, lo, up = READS[matrix]
    o = gu.oracle_run(*read_set(matrix), k, lo, up, threads=8)
    return o.B(), int((np.diff(o.A()["rowptr"]) > 0).sum())


def _engine_case(name):
    matrix, opts, kw, calls, spec = ENGINE_CASES[name]
    oB, nonempty = oracle(matrix)
    if matrix in TRIPLES:
        e = elba_amd.Engine(17, 2, 8, options=opts, **kw)
        M, ncol, rows, cols, vals = TRIPLES[matrix]()
        e.set_kmer_matrix(M, ncol, rows, cols, vals)
    else:
        _, k, lo, up = READS[matrix]
        e = elba_amd.Engine(k, lo, up, options=opts, **kw)
        e.set_reads(*read_set(matrix))
        e.count_kmers()
        e.create_kmer_matrix()
    out = []
    for n, call_opts in enumerate(calls):
        for o, v in call_opts.items():
            e.set_option(o, v)
        st = e.create_seed_matrix()
        B = e.export_csr()
        gu.assert_B_equal(B, oB)
        assert st["rows_lds"] + st["rows_global"] == nonempty, (name, n, st["rows_lds"], st["rows_global"], nonempty)
        got_spec = e.get_stat("overlap_spec")
        if spec is not None:
            assert got_spec == spec, (name, n, got_spec)
        out.append(_record(B, st, got_spec, e.get_stat("overlap_slab_q16") if n in SLAB_Q16_PINNED.get(name, ()) else None))
    e.close()
    return out


def _bounds(lens, world, how):
    if how is None:
        return partition_by_bases(lens, world)
    b = partition_by_bases(lens, 2)       # "empty_middle": three ranks, the second holds no read
    return np.array([b[0], b[1], b[1], b[2]], dtype=np.asarray(b).dtype)


def _shard(packed, off, lens, lo, hi):
    """reads lo .. hi - 1 as a read set of their own"""
    b0 = int(off[lo]) if lo < len(off) else 0
    b1 = int(off[hi - 1]) + (int(lens[hi - 1]) + 3) // 4 if hi > lo else b0
    return np.concatenate([packed[b0:b1], np.zeros(16, np.uint8)]), (off[lo:hi] - np.uint64(b0)), lens[lo:hi]


def _sharded_case(name):
    world, how, nblocks, exchange = SHARDED_CASES[name]
    packed, off, lens = read_set("sharded")
    _, k, lo, up = READS["sharded"]
    oB, nonempty = oracle("sharded")
    bounds = _bounds(lens, world, how)

    def body(rank, h):
        a, b = int(bounds[rank]), int(bounds[rank + 1])
        sp, so, sl = _shard(packed, off, lens, a, b)
        d = DistributedOverlap(k, lo, up, device=0, rank=rank, world=world, dist=h, backend=HipBackend(k, lo, up, 0))
        d.set_reads(sp, so, sl, a, bounds)
        calls = []
        if nblocks == 1:
            d.build_kmer_matrix()
            for n in range(2):           # (a second call on the same panel)
                if exchange == "tiny":
                    d._slot = 4          # a slot too small: _recv returns false, every rank repeats the step with the size that was needed
                st = d.create_seed_matrix(exchange=True if exchange == "tiny" else exchange)
                if exchange == "tiny" and world > 1:
                    assert d._slot > 4, d._slot      # (the step was repeated with the size the headers asked for)
                calls.append((d.export_csr(), st, d.be.e.get_stat("overlap_spec")))
        else:
            d.build_kmer_matrix(row_batches=nblocks)
            for t in range(nblocks):
                d.load_row_block(t)
                st = d.create_seed_matrix()
                calls.append((d.export_csr(), st, d.be.e.get_stat("overlap_spec")))
        d.be.e.close()
        return calls

    parts = dist_sim.run_ranks(world, body)
    if nblocks == 1:
        for n in range(2):
            gu.assert_B_equal(dict(dist_sim.stitch_rows([p[n][0] for p in parts])), oB)
            assert sum(p[n][1]["rows_lds"] + p[n][1]["rows_global"] for p in parts) == nonempty
    else:
        gu.assert_B_equal(dict(dist_sim.stitch_rows([c[0] for p in parts for c in p])), oB)
        assert sum(c[1]["rows_lds"] + c[1]["rows_global"] for p in parts for c in p) == nonempty
    return [[_record(B, st, spec) for (B, st, spec) in p] for p in parts]


def run_case(name):
    """The record of one case: a list of its calls' records (sharded cases: one such list per rank)."""
    return _sharded_case(name) if name in SHARDED_CASES else _engine_case(name)
