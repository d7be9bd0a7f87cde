"""-m gpu: elba_induce_part (elba_amd/csrc/induce.hip), elba_set_overlaps_device and elba_set_outside_counts[_device] (tr.hip) against the
restatement in induce_util.py: the kernels at their own boundaries (read lengths around a byte and a word, one workgroup's 2 KiB of
output, 255 .. 257 reads, 65 535 .. 65 537 pairs, 0 .. 300 straddling pairs on one read), which input the call reads, every error with
its status, and the guarantee: an input assembled part by part on a second context equals the whole run restricted to each part —
flags, S, contigs, cleaned contigs, placements, component counts — and differs on the planted read without the outside counts."""
import ctypes as C

import numpy as np
import pytest

import comp_util as ku
import contig_util as cu
import elba_amd
import induce_util as iu
import string_graph_util as sg
from elba_amd import capi
from oracle import pyoracle as po

pytestmark = pytest.mark.gpu

INVALID, STATE, UNSUPPORTED = 1, 5, 6
NO_PAIRS = (np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64), np.zeros(0, dtype=po.OVERLAP_DTYPE))


@pytest.fixture(scope="module")
def eng():
    e = elba_amd.Engine(17, 2, 8)
    yield e
    e.close()


def _check(e, M, rows, cols, vals, part_of_read, part, reads=None, base=0):
    """induce_part on what the engine holds equals the restatement on (rows, cols, vals, reads); returns (dict, stats)."""
    ind, st = e.induce_part(part_of_read, part, bases=reads is not None)
    want = iu.induce_numpy(M, rows, cols, vals, part_of_read, part, reads)
    assert iu.same_induced(ind, want, reads=reads is not None) is None, iu.same_induced(ind, want, reads=reads is not None)
    assert (st["nreads_in"], st["pairs_in"], st["reads"], st["pairs"], st["packed_bytes"], st["split_pairs"], st["split_passed"], st["id_base"]) == \
           (M, len(rows), want["reads"], want["pairs"], want["packed_bytes"], want["split_pairs"], want["split_passed"], base), st
    assert st["bases"] == (int(np.asarray(reads[2], dtype=np.int64)[want["old_of_new"]].sum()) if reads is not None else 0)
    assert st["ms_total"] >= 0 and st["ms_pairs"] >= 0 and st["ms_gather"] >= 0
    assert (e.get_stat("induce_reads"), e.get_stat("induce_pairs"), e.get_stat("induce_split_pairs")) == (want["reads"], want["pairs"], want["split_pairs"])
    if reads is None:
        assert not (ind["d_packed"] or ind["d_byte_off"] or ind["d_len"]) and ind["packed_bytes"] == 0 and "packed" not in ind
    else:
        pb = ind["packed_bytes"]
        assert ind["packed"][pb:].tolist() == [0] * 16             # the guard bytes
        ends = (want["byte_off"].astype(np.int64) + (want["len"].astype(np.int64) + 3) // 4 - 1)[want["len"] % 4 != 0]
        low = (1 << (2 * (4 - want["len"][want["len"] % 4 != 0].astype(np.int64) % 4))) - 1
        assert ((ind["packed"][ends] & low) == 0).all()           # the unused low bits of every last byte
    return ind, st


def _pairs(rng, M, n, passed=None):
    """n pairs among M reads, ascending in (row, col), with random records."""
    r, c = np.triu_indices(M, 1)
    pick = np.sort(rng.choice(len(r), size=n, replace=False))
    return r[pick].astype(np.int64), c[pick].astype(np.int64), ku.overlap_records(rng, n, po.OVERLAP_DTYPE, passed)


# ---- the rule --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", iu.hand_cases(), ids=lambda c: c[0])
def test_the_rule_one_clause_per_case(eng, case):
    M, rows, cols, vals, part_of_read, part = iu.case_input(case)
    eng.set_overlaps(M, rows, cols, vals)
    ind, st = _check(eng, M, rows, cols, vals, part_of_read, part)
    iu.check_case(case, ind)


def test_selecting_every_read_returns_the_input_and_selecting_none_returns_nothing():
    rng = np.random.default_rng(1)
    seqs = cu.random_reads(rng, 300, 1, 90)
    packed, off, lens = cu.pack(seqs)
    M = len(seqs)
    rows, cols, vals = _pairs(rng, M, 900)
    e, f = elba_amd.Engine(17, 2, 8), elba_amd.Engine(17, 2, 8)
    e.set_reads(packed, off, lens)
    e.set_overlaps(M, rows, cols, vals)
    part_of_read = np.full(M, 4, dtype=np.int32)
    ind, st = _check(e, M, rows, cols, vals, part_of_read, 4, (packed, off, lens))
    pb = int(off[-1]) + (int(lens[-1]) + 3) // 4
    xp, xo, xl = e.export_reads(M, pb)
    assert ind["packed"].tobytes() == xp.tobytes() == packed.tobytes() and (ind["byte_off"] == xo).all() and (ind["len"] == xl).all()
    assert (ind["old_of_new"] == np.arange(M)).all() and (ind["rows"] == rows).all() and (ind["cols"] == cols).all() and ind["vals"].tobytes() == vals.tobytes()
    assert not ind["outside_aligned"].any() and not ind["outside_passed"].any() and st["split_pairs"] == 0
    ind, st = _check(e, M, rows, cols, vals, part_of_read, 5, (packed, off, lens))
    assert (ind["reads"], ind["pairs"], ind["packed_bytes"], st["bases"], st["split_pairs"]) == (0, 0, 0, 0, 0) and ind["packed"].tolist() == [0] * 16
    f.load_part(ind)                                              # ... and loads as a context of 0 reads, like an empty trim
    s = f.transitive_reduction(0.65, 0)
    assert (s["nreads"], s["nedges"], s["nnz"]) == (0, 0, 0) and f.export_string_graph()["n"] == 0
    ind, st = e.induce_part(part_of_read, 4, bases=True, host=False)             # views only
    assert "rows" not in ind and ind["reads"] == M and ind["d_rows"] and ind["d_packed"]
    assert capi._copy_from_device(ind["d_packed"], pb + 16, np.uint8).tobytes() == packed.tobytes()
    assert (capi._copy_from_device(ind["d_cols"], 900, np.int64) == cols).all()
    f.close(); e.close()


# ---- the gather ------------------------------------------------------------------------------------------------------------------------
def test_read_lengths_around_a_byte_and_a_word_under_an_alternating_selection(eng):
    rng = np.random.default_rng(2)
    lens = np.array([0, 1, 3, 4, 5, 7, 8, 9, 31, 32, 33] * 14, dtype=np.uint32)
    lens = rng.permutation(lens)
    lens = np.concatenate([lens[:70], [8192 + 37], lens[70:], [0, 0]]).astype(np.uint32)      # one read longer than a workgroup's 2 KiB of output; reads of 0 bases last
    M = len(lens)
    nb = (lens.astype(np.int64) + 3) // 4
    off = np.concatenate([[0], np.cumsum(nb)[:-1]]).astype(np.uint64)
    packed = rng.integers(0, 256, int(nb.sum()) + 16).astype(np.uint8); packed[-16:] = 0      # (random low bits in the last bytes)
    eng.set_reads(packed, off, lens)
    eng.set_overlaps(M, *NO_PAIRS)
    seen, crowded = set(), 0
    for phase in (0, 1, 2):
        part_of_read = ((np.arange(M) + phase) % 3 != 0).astype(np.int32) if phase else (np.arange(M) % 2).astype(np.int32)
        for part in (0, 1):
            ind, st = _check(eng, M, *NO_PAIRS, part_of_read, part, (packed, off, lens))
            sel = part_of_read == part
            seen |= set((off[sel & (lens > 0)] % 8).tolist())
            words = ind["byte_off"].astype(np.int64)[ind["len"] > 0] // 8
            crowded = max(crowded, int(np.bincount(words).max()))
            assert cu.seqs_of(ind["packed"], ind["byte_off"], ind["len"]) == [s for s, k in zip(cu.seqs_of(packed, off, lens), sel) if k]
    assert seen == set(range(8)) and crowded >= 3                 # source offsets take all eight values mod 8; words hold several reads
    part_of_read = (lens <= 1).astype(np.int32)                   # words of eight reads: only reads of one base (and of none)
    ind, st = _check(eng, M, *NO_PAIRS, part_of_read, 1, (packed, off, lens))
    assert ind["packed_bytes"] == int((lens == 1).sum()) >= 14      # ... up to eight


@pytest.mark.parametrize("nsel", [255, 256, 257])
def test_reads_around_one_workgroup(eng, nsel):
    rng = np.random.default_rng(3)
    M = 2 * nsel + 5
    packed, off, lens = cu.random_packed(rng, M, 1, 40)
    part_of_read = np.zeros(M, dtype=np.int32)
    part_of_read[rng.choice(M, nsel, replace=False)] = 9
    rows, cols, vals = _pairs(rng, M, 2000)
    eng.set_reads(packed, off, lens)
    eng.set_overlaps(M, rows, cols, vals)
    ind, st = _check(eng, M, rows, cols, vals, part_of_read, 9, (packed, off, lens))
    assert ind["reads"] == nsel and st["split_pairs"] > 0 and ind["pairs"] > 0
    ind, st = _check(eng, M, rows, cols, vals, part_of_read, 9)   # without the bases
    eng.set_overlaps(M, *NO_PAIRS)                                # 0 pairs
    ind, st = _check(eng, M, *NO_PAIRS, part_of_read, 9, (packed, off, lens))
    assert ind["reads"] == nsel and ind["pairs"] == 0


@pytest.mark.parametrize("npairs", [255, 256, 257, 65535, 65536, 65537])
def test_kept_pairs_around_one_workgroup_and_two_to_the_16(eng, npairs):
    rng = np.random.default_rng(4)
    M0, M1 = 400, 40                                              # the selected reads hold npairs pairs; the others add pairs that leave and pairs outside
    r0, c0, v0 = _pairs(rng, M0, npairs)
    key = np.unique(rng.integers(0, M0 + M1, 3000) * (M0 + M1) + rng.integers(M0, M0 + M1, 3000))
    r1, c1 = key // (M0 + M1), key % (M0 + M1)
    r1, c1 = r1[r1 < c1], c1[r1 < c1]
    r, c, v = np.concatenate([r0, r1]), np.concatenate([c0, c1]), np.concatenate([v0, ku.overlap_records(rng, len(r1), po.OVERLAP_DTYPE, rng.integers(0, 2, len(r1)))])
    perm = rng.permutation(M0 + M1)
    rows, cols, vals = sg.relabel(perm, r, c, v)
    part_of_read = np.zeros(M0 + M1, dtype=np.int32)
    part_of_read[perm[:M0]] = 1
    eng.set_overlaps(M0 + M1, rows, cols, vals)
    ind, st = _check(eng, M0 + M1, rows, cols, vals, part_of_read, 1)
    assert ind["pairs"] == npairs and st["split_pairs"] > 0 and iu.strictly_ascending(ind["rows"], ind["cols"])


def test_outside_counts_with_0_to_300_straddlers_on_one_read(eng):
    rng = np.random.default_rng(5)
    K = [0, 1, 63, 64, 65, 300, 2]
    M = len(K) + 300
    rr, cc, pp = [], [], []
    for i, k in enumerate(K):
        partners = len(K) + rng.choice(300, k, replace=False)
        rr += [i] * k; cc += partners.tolist(); pp += (rng.random(k) < 0.3).astype(int).tolist()
    rr += [0, 1]; cc += [1, 2]; pp += [1, 0]                       # two pairs inside
    order = np.lexsort((cc, rr))
    rows, cols = np.array(rr, dtype=np.int64)[order], np.array(cc, dtype=np.int64)[order]
    vals = ku.overlap_records(rng, len(rows), po.OVERLAP_DTYPE, np.array(pp, dtype=np.uint8)[order])
    part_of_read = np.zeros(M, dtype=np.int32); part_of_read[:len(K)] = 3
    eng.set_overlaps(M, rows, cols, vals)
    ind, st = _check(eng, M, rows, cols, vals, part_of_read, 3)
    assert ind["outside_aligned"].tolist() == K and ind["pairs"] == 2 and st["split_pairs"] == sum(K)
    assert ind["outside_passed"].tolist() == [int(np.array(pp)[np.array(rr) == i][:K[i]].sum()) for i in range(len(K))]
    ind, st = _check(eng, M, rows, cols, vals, part_of_read, 0)   # from the other side: one straddler per partner pair
    assert st["split_pairs"] == sum(K) and ind["pairs"] == 0


def test_a_selection_that_splits_passed_pairs_is_served_and_counted(eng):
    g = iu.build_input(6, (("layout", 300), ("random", 40), ("layout", 200)), n_failed=50, reads=False)
    rng = np.random.default_rng(6)
    part_of_read = rng.integers(0, 3, g["M"]).astype(np.int32)
    eng.set_overlaps(g["M"], g["rows"], g["cols"], g["vals"])
    total = 0
    for part in range(3):
        ind, st = _check(eng, g["M"], g["rows"], g["cols"], g["vals"], part_of_read, part)
        assert st["split_passed"] > 0 and st["split_passed"] == int(ind["outside_passed"].sum())
        total += st["split_pairs"]
    straddle = part_of_read[g["rows"]] != part_of_read[g["cols"]]
    assert total == 2 * int(straddle.sum())                       # every pair that leaves is counted at both of its ends' parts


# ---- which input the call reads --------------------------------------------------------------------------------------------------------
def test_own_alignments_report_the_id_base_and_a_pruned_list_replaces_them():
    packed, off, lens, info = elba_amd.synth_reads(77, 20000, 10, 2000, 300, error_rate=0.01)
    M = len(lens)
    e = elba_amd.Engine(17, 2, 30)
    e.set_reads(packed, off, lens, first_global_id=1000)
    e.count_kmers(); e.create_kmer_matrix(); e.create_seed_matrix()
    e.align_seeds()
    ov = e.export_overlaps()
    rows, cols, vals = ov["rows"] - 1000, ov["cols"] - 1000, ov["vals"]           # ids are local to the graph's input
    part_of_read = (np.arange(M) % 3).astype(np.int32)
    ind, st = _check(e, M, rows, cols, vals, part_of_read, 1, (packed, off, lens), base=1000)
    assert ind["pairs"] > 0 and st["split_pairs"] > 0
    for min_depth in (3, 6, 10, 15, 25):                          # until some reads, not all, are unsupported
        e.read_pileup(mode=0, margin=0, min_depth=min_depth, min_run=200, trim_len=0)
        flags = e.export_pileup()["flags"]
        if 0 < int((flags & 1 != 0).sum()) < M:
            break
    assert 0 < int((flags & 1 != 0).sum()) < M
    kept = e.prune_reads(1)
    keep = ((flags[rows] & 1) == 0) & ((flags[cols] & 1) == 0)
    assert kept == int(keep.sum()) < len(rows)
    ind, st = _check(e, M, rows[keep], cols[keep], vals[keep], part_of_read, 1, None, base=0)          # the pruned list: a loaded list has no id base
    e.close()


def test_one_context_over_changing_sizes_and_release_workspace(eng):
    rng = np.random.default_rng(8)
    for M, n in ((3000, 20000), (7, 5), (0, 0), (5000, 70000), (40, 0)):
        packed, off, lens = cu.random_packed(rng, M, 0, 50)
        rows, cols, vals = _pairs(rng, M, n) if n else NO_PAIRS
        eng.set_reads(packed, off, lens)
        eng.set_overlaps(M, rows, cols, vals)
        part_of_read = rng.integers(-1, 2, M).astype(np.int32)
        for part in (-1, 0, 1):
            _check(eng, M, rows, cols, vals, part_of_read, part, (packed, off, lens))
        if M == 7:
            eng.release_workspace()                              # the views die, the next call builds them again


# ---- errors ----------------------------------------------------------------------------------------------------------------------------
def _raises(status, f, *a, **kw):
    with pytest.raises(elba_amd.ElbaError) as err:
        f(*a, **kw)
    assert err.value.status == status, (err.value.status, str(err.value))
    return str(err.value)


def test_every_error_status_and_the_state_conditions():
    rng = np.random.default_rng(9)
    e = elba_amd.Engine(17, 2, 8)
    M = 12
    part_of_read = np.zeros(M, dtype=np.int32)
    assert "no overlaps" in _raises(STATE, e.induce_part, part_of_read, 0, bases=False)          # nothing loaded
    _raises(STATE, e.set_outside_counts, np.zeros(M, np.uint32), np.zeros(M, np.uint32))
    _raises(STATE, e.set_outside_counts_device, M, None, None)
    rows, cols, vals = _pairs(rng, M, 20)
    e.set_overlaps(M, rows, cols, vals)
    assert "bases" in _raises(STATE, e.induce_part, part_of_read, 0)                             # the bases without the reads
    e.induce_part(part_of_read, 0, bases=False)
    packed, off, lens = cu.random_packed(rng, M + 1)
    e.set_reads(packed, off, lens)                               # (drops the list)
    e.set_overlaps(M, rows, cols, vals)
    _raises(STATE, e.induce_part, part_of_read, 0)                # reads that are not the graph's
    for kw in (dict(flags=4), dict(flags=-1), dict(reserved=(1, 0)), dict(reserved=(0, 1))):
        _raises(INVALID, e.induce_part, part_of_read, 0, bases=False, **kw)
    _raises(INVALID, e.induce_part, part_of_read[:-1], 0, bases=False)
    _raises(INVALID, e.induce_part, np.zeros(M + 1, np.int32), 0, bases=False)
    o, s = capi.Induced(), capi.InduceStats()
    o.reads, o.pairs = 7, 8                                       # (stale values: the call zeroes them)
    cfg = capi.InduceCfg(0, 0)
    assert e.L.elba_induce_part(e.h, None, part_of_read.ctypes.data, M, C.byref(o), C.byref(s)) == INVALID
    assert o.reads == 0 and o.pairs == 0 and not (o.d_rows or o.rows or o.old_of_new)
    assert e.L.elba_induce_part(e.h, C.byref(cfg), None, M, C.byref(o), C.byref(s)) == INVALID
    assert e.L.elba_induce_part(e.h, C.byref(cfg), part_of_read.ctypes.data, M, None, None) == INVALID
    assert e.L.elba_induce_part(e.h, C.byref(cfg), part_of_read.ctypes.data, M, C.byref(o), None) == 0          # stats are optional
    assert o.reads == M and o.d_rows and not o.rows               # no ELBA_INDUCE_HOST: views only
    e.L.elba_free_induced(C.byref(o))
    # the outside counts
    a, p = np.full(M, 2, np.uint32), np.full(M, 1, np.uint32)
    e.set_outside_counts(a, p)
    for bad_a, bad_p in ((a, a + 1), (np.full(M, 1 << 31, np.uint32), p)):
        assert "passed[v] <= aligned[v]" in _raises(INVALID, e.set_outside_counts, bad_a, bad_p)
    _raises(INVALID, e.set_outside_counts, a[:-1], p[:-1])        # a wrong nreads
    _raises(INVALID, e.set_outside_counts, a, None, nreads=M)     # one array null
    _raises(INVALID, e.set_outside_counts_device, M + 1, None, None)
    e.set_outside_counts(None, None, nreads=M)                    # detach
    e.close()


def test_set_overlaps_device_rejects_the_smallest_offending_index_with_the_hosts_message():
    rng = np.random.default_rng(10)
    M, n = 500, 70000
    rows, cols, vals = _pairs(rng, M, n)
    e, f = elba_amd.Engine(17, 2, 8), elba_amd.Engine(17, 2, 8)
    e.set_overlaps(M, rows, cols, vals)
    whole = np.full(M, 1, dtype=np.int32)
    ind, st = e.induce_part(whole, 1, bases=False)                # the list as device arrays
    f.set_overlaps_device(M, ind["d_rows"], ind["d_cols"], ind["d_vals"], n)
    got, _ = f.induce_part(whole, 1, bases=False)
    assert (got["rows"] == rows).all() and (got["cols"] == cols).all() and got["vals"].tobytes() == vals.tobytes()
    hip = elba_amd.load_library().hipMemcpy
    hip.restype = C.c_int; hip.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]

    def poke(dev, index, value, dtype=np.int64):
        v = np.array([value], dtype=dtype)
        assert hip(int(dev) + v.itemsize * index, v.ctypes.data, v.itemsize, 1) == 0       # hipMemcpyHostToDevice

    def equal_to_predecessor(r, c, a):
        r[a], c[a] = r[a - 1], c[a - 1]                           # not ascending

    def col_is_nreads(r, c, a):
        c[a] = M                                                  # out of range (and still above its predecessor)

    def row_is_col(r, c, a):
        r[a], c[a] = r[a - 1], r[a - 1]                           # out of range and below its predecessor: the range is reported, as by the host loop
    for edits, text in ((((300, equal_to_predecessor), (65537, col_is_nreads)), "ascending"), (((258, col_is_nreads), (65536, equal_to_predecessor)), "row < col"),
                        (((69999, row_is_col),), "row < col"), (((1, equal_to_predecessor), (0, col_is_nreads)), "row < col"), (((256, equal_to_predecessor),), "ascending")):
        r, c = rows.copy(), cols.copy()
        for a, edit in edits:                                     # with two offenders the smaller index is reported, whichever rule it breaks
            edit(r, c, a)
        want = _raises(INVALID, f.set_overlaps, M, r, c, vals)    # the host's message for the same arrays
        assert text in want
        for a, _ in edits:
            poke(ind["d_rows"], a, r[a]); poke(ind["d_cols"], a, c[a])
        msg = _raises(INVALID, f.set_overlaps_device, M, ind["d_rows"], ind["d_cols"], ind["d_vals"], n)
        assert msg == want, (msg, want)
        assert f.induce_part(whole, 1, bases=False)[0]["pairs"] == n            # rejected before `accepted`: the list loaded before stays, as after the host call
        for a, _ in edits:
            poke(ind["d_rows"], a, rows[a]); poke(ind["d_cols"], a, cols[a])
        f.set_overlaps_device(M, ind["d_rows"], ind["d_cols"], ind["d_vals"], n)
    _raises(INVALID, f.set_overlaps_device, M, None, ind["d_cols"], ind["d_vals"], n)
    f.set_overlaps_device(M, None, None, None, 0)
    assert f.induce_part(whole, 1, bases=False)[0]["pairs"] == 0
    # the counts from the device: checked there
    f.set_overlaps_device(M, ind["d_rows"], ind["d_cols"], ind["d_vals"], n)
    f.set_outside_counts_device(M, ind["d_outside_aligned"], ind["d_outside_passed"])          # (of a whole selection: zeros)
    poke(ind["d_outside_passed"], 257, 1, np.uint32)              # passed > aligned
    assert "passed[v] <= aligned[v]" in _raises(INVALID, f.set_outside_counts_device, M, ind["d_outside_aligned"], ind["d_outside_passed"])
    poke(ind["d_outside_aligned"], 257, 1, np.uint32)
    f.set_outside_counts_device(M, ind["d_outside_aligned"], ind["d_outside_passed"])
    poke(ind["d_outside_aligned"], 499, 1 << 31, np.uint32)       # aligned >= 2^31
    _raises(INVALID, f.set_outside_counts_device, M, ind["d_outside_aligned"], ind["d_outside_passed"])
    f.close(); e.close()


# ---- the counts and the bad-read rule ----------------------------------------------------------------------------------------------------
def test_the_counts_enter_the_bad_read_rule_and_are_detached_with_the_list():
    g = iu.build_input(11, (("layout", 200), ("layout", 60), ("layout", 100)), n_failed=60, reads=False)
    M, rows, cols, vals = g["M"], g["rows"], g["cols"], g["vals"]
    rng = np.random.default_rng(11)
    oa = rng.integers(0, 4, M).astype(np.uint32); op = np.minimum(oa, rng.integers(0, 3, M)).astype(np.uint32)
    plain = iu.bad_reads(M, rows, cols, vals).astype(np.uint8)
    counted = iu.bad_reads(M, rows, cols, vals, oa, op).astype(np.uint8)
    assert (plain != counted).any()
    e = elba_amd.Engine(17, 2, 8)

    def bad():
        e.transitive_reduction(0.65, 0)
        return e.export_read_flags(M) & 1
    e.set_overlaps(M, rows, cols, vals)
    assert (bad() == plain).all()
    e.set_outside_counts(oa, op)
    assert (bad() == counted).all() and (bad() == counted).all()  # they stay attached over reductions
    e.set_outside_counts(None, None, nreads=M)
    assert (bad() == plain).all()
    e.set_outside_counts(oa, op)
    e.set_overlaps(M, rows, cols, vals)                           # a new list detaches them
    assert (bad() == plain).all()
    ind, _ = e.induce_part(np.zeros(M, np.int32), 0, bases=False)
    e.set_outside_counts(oa, op)
    e.set_overlaps_device(M, ind["d_rows"], ind["d_cols"], ind["d_vals"], ind["pairs"])
    assert (bad() == plain).all()
    # ... and so does elba_prune_reads: the flags go back to the plain ones of the pruned list
    packed, off, lens = cu.random_packed(rng, M, g["L"], g["L"])
    e.set_reads(packed, off, lens)
    e.set_overlaps(M, rows, cols, vals)
    e.set_outside_counts(oa, op)
    e.read_pileup(mode=0, margin=0, min_depth=1, min_run=1, trim_len=0)
    kept = e.prune_reads(0)                                       # mask 0 prunes nothing: the same pairs, as a new list
    assert kept == len(rows) and (bad() == plain).all()
    e.close()


# ---- the guarantee -----------------------------------------------------------------------------------------------------------------------
GUARANTEE_BLOCKS = (("layout", 900), ("layout", 700), ("layout", 500), ("layout", 400), ("layout", 300), ("layout", 150), ("layout", 40), ("layout", 7))


@pytest.fixture(scope="module")
def whole_run():
    """The built input of about 3000 reads on one engine, and its whole run: computed once, shared, left unchanged."""
    g = iu.build_input(12, GUARANTEE_BLOCKS, n_failed=400, lone=5, p_nodir=1e-12)       # every passed pair has both directions: S holds both images of every pair
    e, second = elba_amd.Engine(17, 2, 8), elba_amd.Engine(17, 2, 8)
    e.set_reads(*g["reads"])
    e.set_overlaps(g["M"], g["rows"], g["cols"], g["vals"])
    whole = iu.late_stages(e, g["M"])
    assert 2900 < g["M"] < 3100 and whole["flags"][g["planted"]] & 1 and whole["S"]["n"] > g["M"]
    entries = set(zip(whole["S"]["rows"].tolist(), whole["S"]["cols"].tolist()))
    assert all((c, r) in entries for r, c in entries)            # ... so the chains are a function of S
    assert sum(c["n"] for c in whole["contigs"]) > 0 and whole["contigs_clean"]["n"] > 0
    yield g, e, second, whole
    second.close(); e.close()


@pytest.mark.parametrize("nparts", [1, 2, 3, 7])
def test_parts_assembled_alone_equal_the_whole_run_restricted(whole_run, nparts):
    g, e, second, whole = whole_run
    part_of_read, runs = iu.assemble_by_parts(e, nparts, second, g["M"], min_reads=1, device=nparts == 3)
    assert (part_of_read >= 0).all() and len(runs) == nparts
    seen = np.zeros(g["M"], dtype=int)
    split = 0
    for part, ind, st, late in runs:
        assert st["split_passed"] == 0 and ind["reads"] > 0
        want = iu.induce_numpy(g["M"], g["rows"], g["cols"], g["vals"], part_of_read, part, g["reads"])
        assert iu.same_induced(ind, want) is None
        assert iu.compare_part(late, whole, ind["old_of_new"]) is None, (part, iu.compare_part(late, whole, ind["old_of_new"]))
        seen[ind["old_of_new"]] += 1
        split += st["split_pairs"]
    assert (seen == 1).all() and (split > 0) == (nparts > 1)
    print("induce_part, %d parts of %d reads, %d pairs: ms_total %s ms_pairs %s ms_gather %s" %
          (nparts, g["M"], len(g["rows"]), *[["%.3f" % st[k] for _, _, st, _ in runs] for k in ("ms_total", "ms_pairs", "ms_gather")]))


def test_flags_and_s_of_parts_where_s_holds_one_image_of_a_pair():
    """Pairs with one direction only (layout_overlaps' p_nodir) leave S with one image of a pair; flags, S and its components are still the
    whole run's restricted.  (The chains are compared on the input without such pairs: on a one-sided S they are not a function of S alone.)"""
    g = iu.build_input(14, GUARANTEE_BLOCKS[2:], n_failed=150, lone=3, p_nodir=0.05)
    e, second = elba_amd.Engine(17, 2, 8), elba_amd.Engine(17, 2, 8)
    e.set_reads(*g["reads"])
    e.set_overlaps(g["M"], g["rows"], g["cols"], g["vals"])
    whole = iu.late_stages(e, g["M"], simplify=None, contigs=False)
    sym = set(zip(whole["S"]["rows"].tolist(), whole["S"]["cols"].tolist()))
    assert any((c, r) not in sym for r, c in sym)                 # the condition, asserted
    for nparts in (2, 5):
        part_of_read, runs = iu.assemble_by_parts(e, nparts, second, g["M"], simplify=None, contigs=False)
        for part, ind, st, late in runs:
            assert st["split_passed"] == 0 and iu.compare_part(late, whole, ind["old_of_new"]) is None, (nparts, part, iu.compare_part(late, whole, ind["old_of_new"]))
    second.close(); e.close()


def test_without_the_counts_the_planted_read_comes_out_different(whole_run):
    g, e, second, whole = whole_run
    x = g["planted"]
    n = e.graph_components("overlaps")[1]["components"]           # as many parts as components: every planted pair leaves its part
    part_of_read, _ = e.partition_components(n, graph="overlaps", min_reads=1, nreads=g["M"])
    ind, st = e.induce_part(part_of_read, int(part_of_read[x]))
    w = int(np.searchsorted(ind["old_of_new"], x))
    assert ind["reads"] == 2 and ind["outside_aligned"][w] == 3 and st["split_passed"] == 0
    second.load_part(ind, outside=False)
    second.transitive_reduction(0.65, 0)
    without = second.export_read_flags(2)
    second.load_part(ind)
    second.transitive_reduction(0.65, 0)
    with_counts = second.export_read_flags(2)
    assert (with_counts == whole["flags"][ind["old_of_new"]]).all() and with_counts[w] & 1 and not without[w] & 1
    assert second.export_string_graph()["n"] == 0                 # the bad read takes its pair with it, as in the whole run ...
    second.load_part(ind, outside=False)
    second.transitive_reduction(0.65, 0)
    assert second.export_string_graph()["n"] == 2                 # ... and without the counts the part assembles a pair the whole run does not have


# ---- end to end --------------------------------------------------------------------------------------------------------------------------
def test_two_genomes_with_a_shared_repeat_from_reads_to_contigs_by_parts():
    """Two genomes that share a repeat of 260 bases (alignments inside it join them: short ones count as containments) beside a third
    that shares nothing: at least two components, pairs of every kind from the aligner itself."""
    rng = np.random.default_rng(13)
    repeat = "".join("ACGT"[x] for x in rng.integers(0, 4, 260))
    seqs = []
    for glen, shared in ((9000, True), (7000, True), (6000, False)):
        body = "".join("ACGT"[x] for x in rng.integers(0, 4, glen))
        genome = body[:glen // 2] + (repeat if shared else "") + body[glen // 2:]
        for start in range(0, len(genome) - 2000, 300):            # overlaps of 1700 .. 500 bases pass, the sixth neighbour's 200 do not
            s = genome[start:start + 2000 + int(rng.integers(0, 100))]
            seqs.append(cu.revcomp(s) if rng.random() < 0.5 else s)
    order = rng.permutation(len(seqs))
    seqs = [seqs[i] for i in order]
    packed, off, lens = cu.pack(seqs)
    M = len(seqs)
    e, second = elba_amd.Engine(17, 2, 40), elba_amd.Engine(17, 2, 40)
    e.set_reads(packed, off, lens)
    e.count_kmers(); e.create_kmer_matrix(); e.create_seed_matrix()
    e.align_seeds()
    ov = e.export_overlaps()
    ncomp = e.graph_components("overlaps")[1]["components"]
    whole = iu.late_stages(e, M, cutoff=0.65, fuzz=100, simplify=(3, 4))
    assert whole["S"]["n"] > 0 and whole["contigs"][3]["n"] >= 2 and ncomp >= 2
    for nparts in (2, 3):
        part_of_read, runs = iu.assemble_by_parts(e, nparts, second, M, min_reads=1, fuzz=100)
        assert sum(r[3] is not None for r in runs) >= 2             # at least two parts with reads
        for part, ind, st, late in runs:
            assert st["split_passed"] == 0
            if late is not None:
                assert iu.compare_part(late, whole, ind["old_of_new"]) is None, (nparts, part, iu.compare_part(late, whole, ind["old_of_new"]))
        print("two genomes: %d reads, %d pairs (%d passed), %d components, parts of %s reads, split pairs %s" %
              (M, ov["n"], int((ov["vals"]["passed"] != 0).sum()), ncomp, [r[1]["reads"] for r in runs], [r[2]["split_pairs"] for r in runs]))
    second.close(); e.close()
