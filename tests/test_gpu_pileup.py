"""-m gpu: read pileups, trimmed intervals, chimera flags and the prune on the GPU (elba_read_pileup / elba_export_pileup / elba_prune_reads,
pileup.hip) against the numpy restatement in pileup_util.py: every segment, trimmed interval, flag and stat."""
import numpy as np
import pytest

import contig_util as cu
import elba_amd
import gpu_util as gu
import pileup_util as pu
import string_graph_util as sgu
from elba_amd.capi import OVERLAP_DTYPE

pytestmark = pytest.mark.gpu

STATS = ("nreads", "pairs", "intervals", "segments", "max_depth", "unsupported", "split", "trimmed", "trimmed_bases")


def _check(e, lens, rows, cols, vals, **cfg):
    st = e.read_pileup(**cfg)
    want, wst, _, _ = pu.pileup(lens, rows, cols, vals, **cfg)
    for k in STATS:
        assert st[k] == wst[k], (k, st[k], wst[k], cfg)
    got = e.export_pileup()
    assert got["n"] == want["n"]
    for k in ("seg_off", "seg_start", "seg_depth", "trim_beg", "trim_end", "flags"):
        assert got[k].shape == want[k].shape and (got[k] == want[k]).all(), (k, cfg)
    assert st["ms_total"] > 0
    return got, st


def _random_overlaps(rng, lens, n, hub=None, hub_n=0, crowd=False):
    """n random pairs (row < col) with intervals inside [0, len]; hub: one read with hub_n extra partners; crowd: many endpoints on few positions."""
    M = len(lens)
    pairs = set()
    while len(pairs) < n:
        a, b = (int(x) for x in rng.integers(0, M, 2))
        if a != b:
            pairs.add((min(a, b), max(a, b)))
    if hub is not None:
        for p in rng.choice(M, size=min(hub_n, M - 1) + 1, replace=False):
            if int(p) != hub:
                pairs.add((min(hub, int(p)), max(hub, int(p))))
    pairs = sorted(pairs)
    rows = np.array([p[0] for p in pairs], np.int64); cols = np.array([p[1] for p in pairs], np.int64)
    vals = np.zeros(len(pairs), OVERLAP_DTYPE)
    for f0, f1, who in (("begQ", "endQ", rows), ("begT", "endT", cols)):
        L = lens[who].astype(np.int64)
        if crowd:
            grid = np.minimum(L, 64)
            x = np.sort(np.stack([rng.integers(0, 5, len(L)) * grid // 4, rng.integers(0, 5, len(L)) * grid // 4], 1), 1)
            x = np.minimum(x, L[:, None])
        else:
            x = np.sort(np.stack([rng.integers(0, L + 1), rng.integers(0, L + 1)], 1), 1)
        vals[f0], vals[f1] = x[:, 0], x[:, 1]
    vals["passed"] = rng.integers(0, 2, len(pairs))
    vals["score"] = rng.integers(-1, 50, len(pairs))
    return rows, cols, vals


def _engine(lens, rows, cols, vals):
    """A context holding random reads of the given lengths and the pair list."""
    rng = np.random.default_rng(3)
    packed = rng.integers(0, 256, int((lens.astype(np.int64) + 3).sum() // 4 + len(lens) + 16)).astype(np.uint8)
    off = np.concatenate([[0], np.cumsum((lens.astype(np.int64) + 3) // 4)])[:-1].astype(np.uint64)
    e = elba_amd.Engine(17, 2, 8)
    e.set_reads(packed, off, lens.astype(np.uint32))
    e.set_overlaps(len(lens), rows, cols, vals)
    return e


@pytest.mark.parametrize("seed", range(6))
def test_random_overlap_lists(seed):
    rng = np.random.default_rng(900 + seed)
    M = int(rng.integers(50, 3000))
    lens = rng.integers(0, 4000, M).astype(np.int64)
    lens[rng.integers(0, M, 3)] = 0                              # reads of length 0
    n = int(rng.integers(M // 4, 4 * M))                          # (some reads get no pair)
    rows, cols, vals = _random_overlaps(rng, lens, n, crowd=seed % 2 == 1)
    e = _engine(lens, rows, cols, vals)
    for mode in (0, 1):
        for margin, md, mr, tl in ((0, 1, 1, 2500), (7, 2, 100, 300), (50, 3, 500, 0)):
            _check(e, lens, rows, cols, vals, mode=mode, margin=margin, min_depth=md, min_run=mr, trim_len=tl)
    e.close()


def test_one_read_with_many_intervals():
    """One read with >= 5 000 partners (the degree of a repeat-rich read) next to ordinary ones, and many endpoints on one position."""
    rng = np.random.default_rng(77)
    M = 12000
    lens = rng.integers(1000, 20000, M).astype(np.int64)
    rows, cols, vals = _random_overlaps(rng, lens, 20000, hub=5, hub_n=8000)
    hub = (rows == 5) | (cols == 5)
    assert hub.sum() >= 5000
    on_q = rows == 5
    vals["begQ"][on_q] = 0; vals["endQ"][on_q] = np.minimum(lens[5], 777)        # the same interval thousands of times
    e = _engine(lens, rows, cols, vals)
    got, st = _check(e, lens, rows, cols, vals, mode=1, margin=0, min_depth=3, min_run=200, trim_len=2500)
    assert st["max_depth"] >= int((on_q & (vals["score"] > 0)).sum())
    _check(e, lens, rows, cols, vals, mode=0, margin=13, min_depth=2, min_run=1000, trim_len=100)
    e.close()


@pytest.mark.parametrize("workload", ["config2", "dense-repeats"])
def test_end_to_end_from_synthetic_reads(workload):
    """count -> B -> align -> pileup on one context equals the restatement on export_overlaps()."""
    if workload == "config2":
        packed, off, lens, info = elba_amd.synth_reads(1, 4_640_000, 30.0, 8240.0, 2000.0, error_rate=0.15, min_len=1000)     # ecsample30x-like
        k, lo, up = 17, 2, 8
    else:
        packed, off, lens, info = elba_amd.synth_reads(4, 1_000_000, 40.0, 10000.0, 1000.0, error_rate=0.01, min_len=1000, repeat_families=20,
                                                       repeat_fraction=0.05, repeat_len=5000)
        k, lo, up = 17, 2, 35
    e, _, _, _ = gu.gpu_full(packed, off, lens, k, lo, up)
    e.align_seeds()
    ov = e.export_overlaps()
    lens = lens.astype(np.int64)
    for mode, margin, md, mr in ((0, 0, 1, 1), (1, 50, 3, 1000), (0, 100, 5, 2000)):
        _check(e, lens, ov["rows"], ov["cols"], ov["vals"], mode=mode, margin=margin, min_depth=md, min_run=mr, trim_len=2500)
    e.close()


def _chimera_reads(seed=51, glen=150_000, nchim=12):
    """Error-free reads of a random genome plus nchim planted chimeras: the first half of one read joined to the second half of a read from
    at least glen / 4 away."""
    packed, off, lens, info = elba_amd.synth_reads(seed, glen, 12, 3000, 500, error_rate=0.0, min_len=1500)
    seqs = cu.seqs_of(packed, off, lens)
    pos = info["genome_pos"]
    n0 = len(seqs)
    rng = np.random.default_rng(seed)
    chim, used = [], set()
    while len(chim) < nchim:
        i, j = (int(x) for x in rng.integers(0, n0, 2))
        if i in used or j in used or abs(int(pos[i]) - int(pos[j])) < glen // 4:
            continue
        used |= {i, j}
        chim.append(seqs[i][:len(seqs[i]) // 2] + seqs[j][len(seqs[j]) // 2:])
    glen_used = int(max(int(pos[v]) + len(seqs[v]) for v in range(n0)))
    g = ["N"] * glen_used
    for v, s in enumerate(seqs):
        fwd = cu.revcomp(s) if info["strand"][v] else s
        g[int(pos[v]):int(pos[v]) + len(fwd)] = fwd
    return seqs + chim, n0, "".join(g)


# Chosen on the CPU with oracle/pyoracle.py's align_upper (the device's alignments) and pileup_util before any GPU run.  With the
# reference's scoring (mismatch / gap -1) an x-drop of 15 runs through a chimeric junction into the unrelated half for hundreds of bases,
# so the alignments of both loci cover the junction and no pileup shows it.  At mismatch / gap -3 (the reads are error-free, so true
# overlaps score the same) a random extension falls 15 below its best within a few bases and both sides' intervals END at the junction
# (the reported end is the best cell).  A margin of 50 then opens a 100-base hole of depth 0 there, while a clean read's interior is
# covered by ~12 reads whose intervals end elsewhere: min_depth 2 and runs of >= 300 bases on both sides flag all 12 planted chimeras
# and none of the 600 clean reads (margins 25 .. 100 and min_depth 1 .. 2 gave the same; min_depth 3 flags 3 clean reads at
# low-coverage spots, margin 0 flags none of the chimeras).  mode 1: the chimeras' overlaps end inside the read and some are not `passed`.
CHIM = dict(mode=1, margin=50, min_depth=2, min_run=300, trim_len=2500)
CHIM_ALIGN = dict(mat=1, mis=-3, gap=-3, dropoff=15)
CLEAN_SPLIT_ALLOWED = 2


def test_planted_chimeras_are_split_and_pruned():
    seqs, n0, G = _chimera_reads()
    Grc = cu.revcomp(G)
    packed, off, lens = cu.pack(seqs)
    e, _, _, _ = gu.gpu_full(packed, off, lens, 17, 2, 40)
    e.align_seeds(**CHIM_ALIGN)
    ov = e.export_overlaps()
    # begT / endT are on T's forward strand also for rc pairs (used as stored): on error-free reads the Q interval is exactly the reverse
    # complement of the T interval
    o = ov["vals"]
    clean = (ov["rows"] < n0) & (ov["cols"] < n0) & (o["score"] > 0)
    for want_rc in (1, 0):
        idx = np.flatnonzero(clean & (o["rc"] == want_rc))
        assert len(idx) > 100
        for a in idx:
            q = seqs[ov["rows"][a]][o["begQ"][a]:o["endQ"][a]]; t = seqs[ov["cols"][a]][o["begT"][a]:o["endT"][a]]
            assert q == (cu.revcomp(t) if want_rc else t), a
    lens64 = lens.astype(np.int64)
    got, st = _check(e, lens64, ov["rows"], ov["cols"], ov["vals"], **CHIM)
    planted = np.arange(n0, len(seqs))
    assert (got["flags"][planted] & 2).all(), got["flags"][planted]
    assert int((got["flags"][:n0] & 2).astype(bool).sum()) <= CLEAN_SPLIT_ALLOWED
    kept = e.prune_reads(2)
    r, c, v = pu.prune(ov["rows"], ov["cols"], ov["vals"], got["flags"], 2)
    assert kept == len(r)
    with pytest.raises(elba_amd.ElbaError) as x:
        e.export_pileup()                                      # the prune invalidates the pileup
    assert x.value.status == 5
    assert e.export_overlaps()["n"] == ov["n"]                 # the alignments stay
    sst = e.transitive_reduction(0.65, 1000)
    _, _, wst = sgu.python_string_graph(len(seqs), r, c, v, 0.65, 1000)
    for k in ("bad_reads", "contained_reads", "edges_kept", "products", "marked", "removed", "nnz"):
        assert sst[k] == wst[k], (k, sst[k], wst[k])
    S = e.export_string_graph()
    pruned = set(np.flatnonzero(got["flags"] & 2).tolist())
    assert not (set(S["rows"].tolist()) | set(S["cols"].tolist())) & pruned
    # the same S as loading the kept pairs by hand
    e2 = elba_amd.Engine(17, 2, 40)
    e2.set_reads(packed, off, lens)
    e2.set_overlaps(len(seqs), r, c, v)
    assert e2.transitive_reduction(0.65, 1000)["nnz"] == sst["nnz"]
    S2 = e2.export_string_graph()
    assert (S2["rows"] == S["rows"]).all() and (S2["cols"] == S["cols"]).all()
    e2.close()
    cst = e.generate_contigs()
    contigs = e.export_contigs()["seqs"]
    assert cst["contigs"] > 0
    bad = [i for i, s in enumerate(contigs) if s not in G and s not in Grc]
    assert not bad, (len(bad), len(contigs))
    e.close()


def test_errors_and_invalidation():
    rng = np.random.default_rng(5)
    lens = rng.integers(100, 500, 40).astype(np.int64)
    rows, cols, vals = _random_overlaps(rng, lens, 100)
    e = elba_amd.Engine(17, 2, 8)
    with pytest.raises(elba_amd.ElbaError) as x:
        e.read_pileup()                                        # nothing aligned, nothing loaded
    assert x.value.status == 5
    e.set_overlaps(len(lens), rows, cols, vals)
    with pytest.raises(elba_amd.ElbaError) as x:
        e.read_pileup()                                        # no reads on the context
    assert x.value.status == 5
    e.close()
    e = _engine(lens, rows, cols, vals)
    for bad in (dict(mode=2), dict(mode=-1), dict(margin=-1), dict(min_depth=0), dict(min_run=0), dict(trim_len=-1)):
        with pytest.raises(elba_amd.ElbaError) as x:
            e.read_pileup(**bad)
        assert x.value.status == 1, bad
    with pytest.raises(elba_amd.ElbaError) as x:
        e.export_pileup()
    assert x.value.status == 5
    with pytest.raises(elba_amd.ElbaError) as x:
        e.prune_reads(1)
    assert x.value.status == 5
    e.read_pileup(mode=1)
    e.export_pileup()
    e.set_overlaps(len(lens), rows, cols, vals)                # a new edge list invalidates it
    with pytest.raises(elba_amd.ElbaError) as x:
        e.export_pileup()
    assert x.value.status == 5
    bad = vals.copy()
    bad["passed"][:] = 1
    bad["endT"][3] = int(lens[cols[3]]) + 1                    # outside [0, len]
    e.set_overlaps(len(lens), rows, cols, bad)
    with pytest.raises(elba_amd.ElbaError) as x:
        e.read_pileup(mode=0)
    assert x.value.status == 1
    bad = vals.copy()
    bad["passed"][:] = 1
    bad["begQ"][7], bad["endQ"][7] = 50, 40                    # beg > end
    e.set_overlaps(len(lens), rows, cols, bad)
    with pytest.raises(elba_amd.ElbaError) as x:
        e.read_pileup(mode=0)
    assert x.value.status == 1
    bad["passed"][7] = 0                                       # ... not credited in mode 0: accepted
    e.set_overlaps(len(lens), rows, cols, bad)
    e.read_pileup(mode=0)
    e.set_reads(*cu.pack(cu.random_reads(rng, 5)))             # a new read set invalidates it
    with pytest.raises(elba_amd.ElbaError) as x:
        e.export_pileup()
    assert x.value.status == 5
    e.close()


def test_new_alignments_invalidate_and_row_shard_fails():
    packed, off, lens, info = elba_amd.synth_reads(8, 60000, 10, 3000, 500, error_rate=0.02, min_len=500)
    e, _, _, _ = gu.gpu_full(packed, off, lens, 17, 2, 12)
    e.align_seeds()
    e.read_pileup()
    e.align_seeds()
    with pytest.raises(elba_amd.ElbaError) as x:
        e.export_pileup()
    assert x.value.status == 5
    e.close()
    # a context that aligned a row shard of B
    from elba_amd.distributed import DistributedOverlap, HipBackend, partition_by_bases
    import dist_sim
    from test_distributed_cpu import _shard
    bounds = partition_by_bases(lens, 2)

    def body(rank, h):
        a, b = int(bounds[rank]), int(bounds[rank + 1])
        d = DistributedOverlap(17, 2, 12, device=0, rank=rank, world=2, dist=h, backend=HipBackend(17, 2, 12, 0))
        d.set_reads(*_shard(packed, off, lens, a, b), a, bounds)
        d.build_kmer_matrix()
        d.create_seed_matrix()
        d.align_seeds()
        try:
            d.be.e.read_pileup()
            status = 0
        except elba_amd.ElbaError as err:
            status = err.status
        d.be.e.close()
        return status

    assert dist_sim.run_ranks(2, body) == [5, 5]


@pytest.mark.parametrize("world", [2, 3])
def test_distributed_pileup_and_prune_equal_one_rank(world):
    """Every rank gathers the aligned pairs (the all-gather of transitive_reduction), computes every read's profile, prunes and reduces:
    profiles, flags and the pruned S equal one rank's."""
    from elba_amd.distributed import DistributedOverlap, HipBackend, partition_by_bases
    import dist_sim
    from test_distributed_cpu import _shard
    reads = elba_amd.synth_reads(34, 100000, 12, 3000, 700, error_rate=0.02, min_len=300)
    packed, off, lens, _ = reads
    cfg = dict(mode=0, margin=20, min_depth=2, min_run=200, trim_len=1000)
    e, _, _, _ = gu.gpu_full(packed, off, lens, 17, 2, 12)
    e.align_seeds()
    st1 = e.read_pileup(**cfg)
    p1 = e.export_pileup()
    kept1 = e.prune_reads(3)
    e.transitive_reduction(0.65, 1000)
    S1 = e.export_string_graph()
    e.close()
    bounds = partition_by_bases(lens, world)

    def body(rank, h):
        a, b = int(bounds[rank]), int(bounds[rank + 1])
        d = DistributedOverlap(17, 2, 12, device=0, rank=rank, world=world, dist=h, backend=HipBackend(17, 2, 12, 0))
        d.set_reads(*_shard(packed, off, lens, a, b), a, bounds)
        d.build_kmer_matrix()
        d.create_seed_matrix()
        d.align_seeds()
        st = d.read_pileup(**cfg)
        p = d.export_pileup()
        kept = d.prune_reads(3)
        d.transitive_reduction(0.65, 1000)
        S = d.export_string_graph()
        d.be.e.close()
        return st, p, kept, S

    for st, p, kept, S in dist_sim.run_ranks(world, body):
        assert all(st[k] == st1[k] for k in STATS)
        for k in ("seg_off", "seg_start", "seg_depth", "trim_beg", "trim_end", "flags"):
            assert (p[k] == p1[k]).all(), k
        assert kept == kept1
        assert (S["rows"] == S1["rows"]).all() and (S["cols"] == S1["cols"]).all() and (S["vals"] == S1["vals"]).all()
