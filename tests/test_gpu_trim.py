"""-m gpu: reads cut to their supported intervals and chimeras split on the GPU (elba_trim_reads / elba_export_trim_map /
elba_get_trimmed_reads_device / elba_adopt_trimmed_reads, trim.hip) against the numpy restatement in trim_util.py: every byte of the packed
buffer and its guard, every offset, length, map entry and stat."""
import numpy as np
import pytest

import contig_util as cu
import elba_amd
import gpu_util as gu
import pileup_util as pu
import string_graph_util as sgu
import trim_util as tu
from test_gpu_pileup import _engine, _random_overlaps

pytestmark = pytest.mark.gpu

RUNS = dict(mode=1, margin=0, min_depth=1, min_run=1, trim_len=0)      # every credited interval is a run of its own, if a gap separates them


def _source(lens):
    """The packed bytes test_gpu_pileup._engine gives a context for these lengths (random bytes: the reads' own padding bits are garbage)."""
    rng = np.random.default_rng(3)
    packed = rng.integers(0, 256, int((lens.astype(np.int64) + 3).sum() // 4 + len(lens) + 16)).astype(np.uint8)
    off = np.concatenate([[0], np.cumsum((lens.astype(np.int64) + 3) // 4)])[:-1].astype(np.uint64)
    return packed, off


def _assert_reads(got, want, what):
    packed, off, ln = got
    assert ln.shape == want["len"].shape and (ln == want["len"]).all(), what
    assert (off == want["byte_off"]).all(), what
    assert packed.shape == want["packed"].shape, (what, packed.shape, want["packed"].shape)
    bad = np.flatnonzero(packed != want["packed"])
    assert len(bad) == 0, (what, "first differing byte", int(bad[0]), len(bad))
    assert not packed[len(packed) - 16:].any(), what


def _check(e, want, wst, mode, min_len, adopt=False):
    """One elba_trim_reads call on a context with a valid pileup against the restatement's result; with adopt, also through export_reads."""
    st = e.trim_reads(mode=mode, min_len=min_len)
    for k in tu.STATS:
        assert st[k] == wst[k], (k, st[k], wst[k], mode, min_len)
    assert st["ms_total"] > 0 and st["ms_repack"] >= 0
    m = e.export_trim_map()
    assert m["n"] == want["n"]
    for k in ("src_read", "src_beg", "src_end"):
        assert m[k].dtype == want[k].dtype and (m[k] == want[k]).all(), (k, mode, min_len)
    v = e.trimmed_reads_device()
    assert v["n"] == want["n"] and v["packed_bytes"] == wst["packed_bytes"]
    _assert_reads((gu.host_copy(v["d_packed"], v["packed_bytes"] + 16, np.uint8), gu.host_copy(v["d_byte_off"], v["n"], np.uint64),
                   gu.host_copy(v["d_len"], v["n"], np.uint32)), want, ("device", mode, min_len))
    if adopt:
        e.adopt_trimmed_reads()
        _assert_reads(e.export_reads(want["n"], wst["packed_bytes"]), want, ("adopted", mode, min_len))
    return st, m


def _hand_case(lens, intervals, mode=1, min_len=1, cfg=RUNS, adopt=True, packed=None):
    lens = np.asarray(lens, dtype=np.int64)
    rows, cols, vals = tu.overlaps_for(len(lens), intervals)
    if packed is None:
        packed, off = _source(lens)
        e = _engine(lens, rows, cols, vals)
    else:
        packed, off = packed
        e = elba_amd.Engine(17, 2, 8)
        e.set_reads(packed, off, lens.astype(np.uint32))
        e.set_overlaps(len(lens), rows, cols, vals)
    e.read_pileup(**cfg)
    want, wst = tu.trim(packed, off, lens, rows, cols, vals, cfg, mode=mode, min_len=min_len)
    st, m = _check(e, want, wst, mode, min_len, adopt=adopt)
    return e, want, wst, (packed, off)


LATTICE_LENS = (1, 2, 3, 4, 5, 7, 8, 9, 31, 32, 33, 63, 64, 65)


def test_alignment_lattice():
    """Pieces of every length in LATTICE_LENS at every beg mod 4, from sources at every byte offset mod 8 to destinations at every byte
    offset mod 8 (asserted from the map below); the sources are random bytes."""
    lens, intervals = [], []
    for rep in range(3):
        for i, L in enumerate(LATTICE_LENS):
            r, cur = len(lens), 0
            for k in range(4):
                res = (k + rep) % 4
                beg = cur + 1 + (res - (cur + 1)) % 4                 # the first base past a gap of >= 1 with beg mod 4 == res
                intervals.append((r, beg, beg + L)); cur = beg + L
            lens.append(cur + (i + rep) % 5)                          # 0 .. 4 bases behind the last piece
    e, want, wst, (packed, off) = _hand_case(lens, intervals)
    assert want["n"] == len(intervals) and [(int(a), int(b), int(c)) for a, b, c in zip(want["src_read"], want["src_beg"], want["src_end"])] == intervals
    combos = {(int(b) % 4, int(c - b)) for b, c in zip(want["src_beg"], want["src_end"])}
    assert combos == {(r, L) for r in range(4) for L in LATTICE_LENS}
    assert {int(off[r]) % 8 for r in want["src_read"]} == set(range(8))
    assert {int(o) % 8 for o in want["byte_off"]} == set(range(8))
    assert {(int(off[r]) + int(b) // 4) % 8 for r, b in zip(want["src_read"], want["src_beg"])} == set(range(8))      # the first source byte of a piece
    # the adopted pieces are a read set like any other: they can be counted
    assert e.count_kmers()["nreads"] == want["n"]
    e.close()


def test_last_base_of_the_buffer_empty_reads_and_reads_without_pairs():
    lens = [0, 37, 50, 0, 1, 29]                                      # read 1 has no pair at all; reads 0 and 3 have no bases
    intervals = [(2, 3, 20), (2, 21, 50), (4, 0, 1), (5, 6, 29)]      # the last piece ends at the last base of the last read of the buffer
    e, want, wst, _ = _hand_case(lens, intervals)
    assert wst["pieces"] == 4 and wst["reads_dropped"] == 3 and wst["reads_split"] == 1 and wst["reads_unchanged"] == 1
    e.close()
    # mode 0 on the same pileup: GetTrimmedInterval's best run of each read (trim_len 0)
    e, want, wst, _ = _hand_case(lens, intervals, mode=0)
    assert wst["pieces"] == 3
    e.close()


def test_every_read_dropped_gives_an_empty_read_set():
    """Pinned: no piece is no error.  n = 0, packed_bytes = 0, the 16 guard bytes exist and are zero, adopt leaves a context with 0 reads."""
    lens = [40, 50, 60]
    e, want, wst, _ = _hand_case(lens, [(0, 2, 30), (1, 0, 50)], min_len=1000, adopt=False)
    assert want["n"] == 0 and wst["packed_bytes"] == 0 and wst["reads_dropped"] == 3
    v = e.trimmed_reads_device()
    assert v["n"] == 0 and v["packed_bytes"] == 0 and v["d_packed"]
    assert not gu.host_copy(v["d_packed"], 16, np.uint8).any()
    e.adopt_trimmed_reads()
    packed, off, ln = e.export_reads(0, 0)
    assert len(off) == 0 and len(ln) == 0 and not packed.any()
    assert e.count_kmers()["nreads"] == 0
    e.close()


@pytest.mark.parametrize("mode", [0, 1])
def test_nothing_trimmed_returns_the_input_byte_for_byte(mode):
    rng = np.random.default_rng(12)
    seqs = cu.random_reads(rng, 60, lo=1, hi=300)
    packed, off, lens = cu.pack(seqs)                                # padding bits zero
    # the whole read once and its last base twice: one run, and the average depth of [0, i] is largest at the last base, so that
    # GetTrimmedInterval's best run is the whole read as well
    intervals = [iv for r, L in enumerate(lens) for iv in ((r, 0, int(L)), (r, int(L) - 1, int(L)))]
    e, want, wst, _ = _hand_case(lens, intervals, mode=mode, packed=(packed, off))
    assert wst["reads_unchanged"] == 60 and wst["bases_out"] == wst["bases_in"]
    assert (want["packed"] == packed).all() and (want["byte_off"] == off).all() and (want["len"] == lens).all()
    e.close()


def test_one_long_piece_between_thousands_of_one_base_pieces():
    lens = np.full(2600, 3, np.int64)
    lens[0] = lens[2] = 5001; lens[1] = 70010
    intervals = [(0, 2 * i, 2 * i + 1) for i in range(2500)] + [(1, 1, 70004)] + [(2, 2 * i + 1, 2 * i + 2) for i in range(2500)]
    e, want, wst, _ = _hand_case(lens, intervals)
    assert wst["pieces"] == 5001 and wst["longest"] == 70003
    e.close()


def test_one_read_with_hundreds_of_long_runs():
    rng = np.random.default_rng(8)
    intervals, cur = [], 0
    for i in range(320):
        beg = cur + int(rng.integers(1, 4)); end = beg + int(rng.integers(5, 40)); cur = end
        intervals.append((1, beg, end))
    lens = np.full(330, 10, np.int64); lens[1] = cur + 2
    cfg = dict(RUNS, min_run=5)
    e, want, wst, _ = _hand_case(lens, intervals, cfg=cfg, adopt=False)
    assert wst["pieces"] == 320 and wst["reads_split"] == 1
    _check(e, *tu.trim(*_source(lens), lens, *tu.overlaps_for(330, intervals), cfg, mode=1, min_len=20), 1, 20)      # some of the runs dropped
    e.close()


def test_more_pieces_than_lanes_of_the_count_kernel():
    """k_trim_count runs one lane per read: 40 reads are one block of 256 lanes, their 1200 pieces more than four times that."""
    intervals = [(r, 3 * i + (r % 3), 3 * i + (r % 3) + 2) for r in range(40) for i in range(30)]
    lens = np.full(40, 95, np.int64)
    e, want, wst, _ = _hand_case(lens, intervals)
    assert wst["pieces"] == 1200 > 256
    e.close()


@pytest.mark.parametrize("seed", range(6))
def test_random_overlap_lists(seed):
    """test_gpu_pileup.test_random_overlap_lists' lists and pileup parameters; both trim modes, min_len 1, 17 and 500."""
    rng = np.random.default_rng(900 + seed)
    M = int(rng.integers(50, 3000))
    lens = rng.integers(0, 4000, M).astype(np.int64)
    lens[rng.integers(0, M, 3)] = 0
    n = int(rng.integers(M // 4, 4 * M))
    rows, cols, vals = _random_overlaps(rng, lens, n, crowd=seed % 2 == 1)
    e = _engine(lens, rows, cols, vals)
    packed, off = _source(lens)
    for i, (margin, md, mr, tl) in enumerate(((0, 1, 1, 2500), (7, 2, 100, 300), (50, 3, 500, 0))):
        cfg = dict(mode=(seed + i) % 2, margin=margin, min_depth=md, min_run=mr, trim_len=tl)
        e.read_pileup(**cfg)
        pile = pu.pileup(lens, rows, cols, vals, **cfg)
        for mode in (0, 1):
            for min_len in (1, 17, 500):
                _check(e, *tu.trim_of(packed, off, lens, pile, cfg, mode=mode, min_len=min_len), mode, min_len)
    e.close()


def _status(f, *a, **kw):
    with pytest.raises(elba_amd.ElbaError) as x:
        f(*a, **kw)
    return x.value.status


def test_errors_and_invalidation():
    rng = np.random.default_rng(5)
    lens = rng.integers(100, 500, 40).astype(np.int64)
    rows, cols, vals = _random_overlaps(rng, lens, 100)
    cfg = dict(mode=1, margin=0, min_depth=1, min_run=20, trim_len=50)
    e = _engine(lens, rows, cols, vals)
    packed, off = _source(lens)
    # no pileup yet
    assert _status(e.trim_reads) == 5
    for f in (e.export_trim_map, e.trimmed_reads_device, e.adopt_trimmed_reads):
        assert _status(f) == 5
    e.read_pileup(**cfg)
    for bad in (dict(mode=2), dict(mode=-1), dict(min_len=0), dict(min_len=-3), dict(reserved=(1, 0)), dict(reserved=(0, 7))):
        assert _status(e.trim_reads, **bad) == 1, bad
    assert _status(e.export_trim_map) == 5                            # a failed call leaves no trimmed reads
    want, wst = tu.trim(packed, off, lens, rows, cols, vals, cfg, mode=1, min_len=10)
    _check(e, want, wst, 1, 10)
    # the snapshot survives the prune (which invalidates the pileup) and the release of the workspace
    e.prune_reads(2)
    assert _status(e.export_pileup) == 5
    e.release_workspace()
    m = e.export_trim_map()
    assert (m["src_read"] == want["src_read"]).all() and (m["src_beg"] == want["src_beg"]).all()
    _assert_reads(e.export_trimmed_reads(), want, "after prune and release")
    assert _status(e.trim_reads) == 5                                 # ... but a new trim needs a valid pileup
    assert _status(e.export_trim_map) == 5
    # a new pileup invalidates it
    e.set_overlaps(len(lens), rows, cols, vals)
    e.read_pileup(**cfg)
    e.trim_reads(mode=1, min_len=10)
    e.read_pileup(**cfg)
    for f in (e.export_trim_map, e.trimmed_reads_device, e.adopt_trimmed_reads):
        assert _status(f) == 5
    # a new read set invalidates it
    e.trim_reads(mode=0, min_len=1)
    e.set_reads(packed, off, lens.astype(np.uint32))
    for f in (e.export_trim_map, e.trimmed_reads_device, e.adopt_trimmed_reads):
        assert _status(f) == 5
    assert _status(e.trim_reads) == 5                                 # (the read set took the pileup with it)
    # adopt consumes it, and everything derived from the old reads goes the way elba_set_reads sends it
    e.set_overlaps(len(lens), rows, cols, vals)
    e.read_pileup(**cfg)
    _check(e, want, wst, 1, 10, adopt=True)
    for f in (e.export_trim_map, e.trimmed_reads_device, e.adopt_trimmed_reads, e.export_pileup):
        assert _status(f) == 5
    assert _status(e.read_pileup) == 5 and _status(e.transitive_reduction, 0.65, 1000) == 5      # the loaded edge list is gone
    e.close()
    # pairs alone, no reads: there is no pileup to cut by
    e = elba_amd.Engine(17, 2, 8)
    e.set_overlaps(len(lens), rows, cols, vals)
    assert _status(e.trim_reads) == 5
    e.close()


def test_planted_chimeras_are_split_and_the_pieces_assemble():
    """Conditions, checked on the CPU before any GPU run with oracle/pyoracle.py's align_upper (CHIM_ALIGN), pileup_util and trim_util on the
    same reads: with CHIM and min_len 300 every one of the 12 planted chimeras gave exactly two pieces, no clean read was split or dropped
    (624 pieces of 612 reads), every piece was a substring of the genome or its reverse complement, and the pieces' string graph gave one
    contig of 149 695 bases inside the genome.  Nothing had to be changed: the first parameters tried (test_gpu_pileup.py's own) held."""
    seqs, n0, G = tu.chimera_reads(elba_amd.synth_reads)
    Grc = cu.revcomp(G)
    assert not [s for s in seqs[n0:] if s in G or s in Grc]            # no whole chimera is a substring
    packed, off, lens = cu.pack(seqs)
    e, _, _, _ = gu.gpu_full(packed, off, lens, 17, 2, 40)
    e.align_seeds(**tu.CHIM_ALIGN)
    ov = e.export_overlaps()
    e.read_pileup(**tu.CHIM)
    want, wst = tu.trim(packed, off, lens.astype(np.int64), ov["rows"], ov["cols"], ov["vals"], tu.CHIM, mode=1, min_len=300)
    st, m = _check(e, want, wst, 1, 300, adopt=True)
    per = np.bincount(m["src_read"], minlength=len(seqs))
    assert (per[n0:] >= 2).all(), per[n0:]
    assert int((per[:n0] >= 2).sum()) <= tu.CLEAN_SPLIT_ALLOWED
    pieces = cu.seqs_of(want["packed"], want["byte_off"], want["len"])
    assert pieces == [seqs[r][b:c] for r, b, c in zip(m["src_read"], m["src_beg"], m["src_end"])]
    bad = [i for i, s in enumerate(pieces) if s not in G and s not in Grc]
    assert not bad, (len(bad), len(pieces))
    # the pipeline again, on the pieces: no prune this time
    n = len(pieces)
    assert e.count_kmers()["nreads"] == n
    e.create_kmer_matrix(); e.create_seed_matrix()
    e.align_seeds(**tu.CHIM_ALIGN)
    ov2 = e.export_overlaps()
    sst = e.transitive_reduction(0.65, 1000)
    _, _, ost = sgu.python_string_graph(n, ov2["rows"], ov2["cols"], ov2["vals"], 0.65, 1000)
    for k in ("bad_reads", "contained_reads", "edges_kept", "products", "marked", "removed", "nnz"):
        assert sst[k] == ost[k], (k, sst[k], ost[k])
    cst = e.generate_contigs()
    contigs = e.export_contigs()["seqs"]
    assert cst["contigs"] >= 1
    badc = [i for i, s in enumerate(contigs) if s not in G and s not in Grc]
    assert not badc, (len(badc), len(contigs))
    e.close()


@pytest.mark.parametrize("world", [2, 3])
def test_distributed_trim_equals_one_rank(world):
    """Every rank cuts the replicated reads by the gathered pileup: the map and the bytes on every rank equal one rank's."""
    from elba_amd.distributed import DistributedOverlap, HipBackend, partition_by_bases
    import dist_sim
    from test_distributed_cpu import _shard
    packed, off, lens, _ = elba_amd.synth_reads(34, 100000, 12, 3000, 700, error_rate=0.02, min_len=300)
    cfg = dict(mode=0, margin=20, min_depth=2, min_run=200, trim_len=1000)
    e, _, _, _ = gu.gpu_full(packed, off, lens, 17, 2, 12)
    e.align_seeds()
    e.read_pileup(**cfg)
    one = {}
    for mode in (0, 1):
        st = e.trim_reads(mode=mode, min_len=100)
        one[mode] = (st, e.export_trim_map(), e.export_trimmed_reads())
        assert st["pieces"] > 100
    e.close()
    bounds = partition_by_bases(lens, world)

    def body(rank, h):
        a, b = int(bounds[rank]), int(bounds[rank + 1])
        d = DistributedOverlap(17, 2, 12, device=0, rank=rank, world=world, dist=h, backend=HipBackend(17, 2, 12, 0))
        d.set_reads(*_shard(packed, off, lens, a, b), a, bounds)
        d.build_kmer_matrix()
        d.create_seed_matrix()
        d.align_seeds()
        d.read_pileup(**cfg)
        out = [d.trim_reads(mode=mode, min_len=100) for mode in (0, 1)]
        d.be.e.close()
        return out

    for out in dist_sim.run_ranks(world, body):
        for mode in (0, 1):
            st1, m1, (p1, o1, l1) = one[mode]
            got = out[mode]
            assert all(got["stats"][k] == st1[k] for k in tu.STATS)
            for k in ("src_read", "src_beg", "src_end"):
                assert (got[k] == m1[k]).all(), k
            assert (got["packed"] == p1).all() and (got["byte_off"] == o1).all() and (got["len"] == l1).all()
