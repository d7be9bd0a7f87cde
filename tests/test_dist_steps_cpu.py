"""CPU tests of the scripted worlds of tests/dist_step_cases.py: every case's CLAIMS (the properties that make it hit its edge, so that a
change to a generator cannot turn a case into a trivial one unnoticed), the scripts against the one-rank oracle (NumpyBackend at 64 ranks,
with empty ranks and hand-set owner ranges), the replay harness against the scripts, and the comparison rules against what they must reject."""
import numpy as np
import pytest

import dist_sim
import dist_step_cases as dsc
from elba_amd.distributed import kmer_words
from oracle import pyoracle as po

ALL = sorted(dsc.CASES)


def _instances(c):
    return [int(c.inst_off(r)[-1]) for r in range(c.W)]


def _bits(x):
    return max(1, int(x).bit_length())


@pytest.mark.parametrize("name", ALL)
def test_stitched_rows_of_the_script_equal_the_one_rank_oracle(name):
    sc = dsc.script(name)
    c = sc.case
    o = po.Oracle(c.k, c.lower, c.upper)
    o.count_and_build(c.packed, c.off, c.lens)
    o.spgemm(2)
    B, oB = dist_sim.stitch_rows(sc.steps["rows"]), o.B()
    assert B["Y"] == oB["Y"] and (B["rowptr"] == oB["rowptr"]).all() and (B["col"] == oB["col"].astype(np.int64)).all() and (B["val"] == oB["val"]).all()
    assert sum(s[2] for s in sc.steps["kstats"]) == o.stat("N") == sc.n_total and sum(s[3] for s in sc.steps["kstats"]) == o.stat("Z")
    assert sum(s[0] for s in sc.steps["kstats"]) == o.stat("I") == sum(_instances(c))
    # sizes: the numpy side loops per read and per column
    assert len(c.seqs) <= 400 and o.stat("I") <= 60000 and o.stat("N") <= 20000
    if c.W < 64 and not name.startswith("packed_k"):
        assert max(_instances(c)) > 4096          # three or more enumeration blocks of 2048, the last one partial
        assert max(_instances(c)) % 2048 != 0
    if name != "packed_k5":
        assert oB["Y"] >= 10                      # (the reads do overlap: B is not trivial)


@pytest.mark.parametrize("name", ALL)
def test_replay_on_a_second_numpy_backend_reproduces_the_script(name):
    sc = dsc.script(name)
    c = sc.case
    for r in range(c.W):
        out = dsc.replay(dist_sim.NumpyBackend(c.k, c.lower, c.upper), sc, r, check=dsc.checker(sc, r))
        assert set(out) == set(sc.steps) - {"gid"}


# ---- claims -----------------------------------------------------------------------------------------------------------------------
def test_claims_short_reads():
    c = dsc.script("short_reads").case
    k = c.k
    sl = [c.lens[int(c.bounds[r]):int(c.bounds[r + 1])].astype(np.int64) for r in range(3)]
    io = [c.inst_off(r) for r in range(3)]
    assert sorted(set(sl[0][:4].tolist())) == [1, k - 1, k, k + 1] and sorted(set(sl[2][-4:].tolist())) == [1, k - 1, k, k + 1]
    assert io[0][0] == io[0][1] == io[0][2] == 0 and io[0][3] == 1            # shard 0: instance 0 lies in the THIRD read
    assert io[2][-1] == io[2][-2]                                              # shard 2: the last read has no instance
    short = sl[1] < k
    I = int(io[1][-1])
    runs = []                                                                  # (first read, reads) of every run of reads shorter than k in shard 1
    j = 0
    while j < len(short):
        if short[j]:
            e = j
            while e < len(short) and short[e]:
                e += 1
            runs.append((j, e - j)); j = e
        else:
            j += 1
    at_wave = [(j, n) for j, n in runs if n >= 3 and 0 < io[1][j] < I and io[1][j] % 512 == 0]
    assert at_wave, "a run of >= 3 short reads whose next instance is a wavefront's first"
    mid_wave = [(j, n) for j, n in runs if 0 < io[1][j] < I and io[1][j] % 512 != 0]
    assert mid_wave, "a run of short reads that a wavefront's forward walk has to cross"
    starts = np.arange(512, I, 512)
    assert (~np.isin(starts, io[1])).any(), "a wavefront that starts inside a read"
    assert {k, k + 1} <= set(sl[1].tolist())


def test_claims_empty_ranks():
    sc = dsc.script("empty_ranks")
    c = sc.case
    assert np.diff(c.bounds).tolist() == [0, 40, 0, 5, 0]
    assert [n > 0 for n in _instances(c)] == [False, True, False, False, False]
    assert (c.lens[int(c.bounds[3]):int(c.bounds[4])] < c.k).all()
    oc, pc = np.array(sc.steps["owner_counts"]), np.array(sc.steps["panel_counts"])
    # rank 1 sends instances to other owners and gets columns back from them; rank 3 (reads, no instance) owns k-mers of rank 1's reads
    assert (oc[1, [0, 2, 3, 4]] > 0).all() and (pc[[0, 2, 3, 4], 1] > 0).all()
    assert oc[[0, 2, 3, 4]].sum() == 0 and pc[:, [0, 2, 3, 4]].sum() == 0
    assert all(s[2] > 0 for s in sc.steps["kstats"])                          # every rank, with reads or without, owns reliable k-mers


@pytest.mark.parametrize("name", ["owners_64_hist", "owners_64_hand"])
def test_claims_owners_64(name):
    sc = dsc.script(name)
    c = sc.case
    u = sc.upper_bins.astype(np.int64)
    h = np.sum(sc.steps["hist"], axis=0)
    assert c.W == 64 and len(u) == 64 and u[-1] == 4096
    inner = [r for r in range(63) if 0 < u[r] < 4096 and h[u[r] - 1] > 0 and h[u[r]] > 0]
    assert len(inner) >= 8, "boundaries with instances in the bin on either side"
    got = np.array([rc.sum() for rc in sc.recv_counts])
    width = np.diff(np.concatenate([[0], u]))
    assert (got[width == 0] == 0).all()
    if name == "owners_64_hand":
        assert u[0] == 0 and u[31] == u[30] and u[62] == 4096
        assert (width == 0).sum() >= 3 and {0, 31, 63} <= set(np.flatnonzero(width == 0).tolist())
        assert got[1] > 0 and got[32] > 0 and got[62] > 0 and got[30] > 0
        assert {0, 1, 31, 32, 62, 63} <= set(c.device_ranks)
    else:
        assert (got > 0).all() and {0, 31, 62, 63} <= set(c.device_ranks)
    # every owner is sent to from more than one rank, every sender uses most owners: the LDS tables of 64 counters are all in use
    assert min(np.count_nonzero(oc) for oc in sc.steps["owner_counts"]) > 32


@pytest.mark.parametrize("name,per_rank,fmt", [("packed_k27_fits", 2048, (53, 11)), ("packed_k27_over", 2049, None), ("packed_k31_fits", 256, (56, 8)),
                                               ("packed_k31_over", 257, None), ("packed_k7", None, (14, None)), ("packed_k5", None, None)])
def test_claims_packed_limit(name, per_rank, fmt):
    sc = dsc.script(name)
    c = sc.case
    assert c.W == dict(k27=2, k31=64, k7=1, k5=2)[name.split("_")[1]]
    if per_rank is not None:
        assert max(_instances(c)) == per_rank
        width = np.diff(np.concatenate([[0], sc.upper_bins.astype(np.int64)]))
        assert (width == 4096 // c.W).all()
    if fmt is not None and fmt[1] is None:
        fmt = (14, _bits(max(_instances(c)) - 1))
    assert sc.fmt == fmt
    assert ("send8" in sc.steps) == (fmt is not None)
    if fmt is not None and per_rank is not None:
        assert fmt[0] + fmt[1] == 64                                           # exactly at the limit


@pytest.mark.parametrize("k", [33, 65])
def test_claims_multiword(k):
    sc = dsc.script("multiword_%d" % k)
    c = sc.case
    kw = kmer_words(k)
    assert kw == (2 if k == 33 else 3) and c.W == (3 if k == 33 else 2)
    words = []
    for tail in (b"A", b"C"):
        buf, _, _ = po.pack_reads([c.stem + tail])
        w = np.zeros(3, dtype=np.uint64)
        po.lib().orc_kmerN_at(buf.ctypes.data, 0, k, w.ctypes.data)
        words.append(w[:kw].copy())
    assert (words[0][:kw - 1] == words[1][:kw - 1]).all() and words[0][kw - 1] != words[1][kw - 1]     # they differ past base 32 / 64 only
    owners = [[r for r in range(c.W) if (sc.steps["rel"][r] == w).all(axis=1).any()] for w in words]
    assert len(owners[0]) == 1 and owners[0] == owners[1], "both planted k-mers are reliable and live on one owner"
    rel = sc.steps["rel"][owners[0][0]]
    lead = rel[:, :kw - 1]
    assert (np.diff(lead, axis=0) == 0).all(axis=1).sum() >= 1                 # neighbours of the sorted list that share all leading words
    assert all(len(s) and s.shape[1] == kw + 1 for s in sc.steps["send"][0])   # 24- / 32-byte records to every owner


@pytest.mark.parametrize("lower,upper", [(2, 4), (3, 3), (2, 40)])
def test_claims_count_edges(lower, upper):
    sc = dsc.script("count_edges_%d_%d" % (lower, upper))
    c = sc.case
    ok = False
    for r in range(c.W):
        _, cnt = np.unique(sc.recv16[r][:, 0], return_counts=True)
        ok |= set(range(lower - 1, upper + 2)) <= set(cnt.tolist())
        if upper == 40:
            assert ((cnt >= 33) & (cnt <= 40)).any(), "a column of at least 33 entries on every owner"
    assert ok, "one owner sees every count from LOWER - 1 to UPPER + 1"
    twice = False
    for r in range(c.W):
        p = np.concatenate(sc.steps["panel_send"][r])
        p = p[np.lexsort((p[:, 1], p[:, 0]))]
        twice |= bool(((p[1:, 0] == p[:-1, 0]) & ((p[1:, 1] >> np.uint64(32)) == (p[:-1, 1] >> np.uint64(32)))).any())
    assert twice, "some read holds a reliable k-mer twice"
    # the three arrival orders give the same columns, statistics and reliable k-mers (the restatement; the device: test_gpu_dist_steps.py)
    for r in range(c.W):
        ref = None
        for name, order in dsc.record_orders(len(sc.recv16[r])).items():
            be = dist_sim.NumpyBackend(c.k, c.lower, c.upper)
            st = be.count_records(dsc._t(be, sc.recv16[r][order], 2))
            got = (tuple(st[f] for f in dsc.STAT_FIELDS), be.rel.tolist(), [x.tolist() for x in be.cols])
            ref = ref or got
            assert got == ref, name
        assert ref[0] == sc.steps["kstats"][r]


@pytest.mark.parametrize("W", [64, 3])
def test_claims_panel_windows(W):
    sc = dsc.script("panel_windows_%d" % W)
    c = sc.case
    b = c.bounds
    rank_of = lambda reads: np.searchsorted(b, reads.astype(np.int64), side="right") - 1
    # a column with reads of rank 0 and of rank W - 1 and of no rank in between
    found = False
    for r in range(W):
        p = np.concatenate(sc.steps["panel_send"][r])
        if not len(p):
            continue
        p = np.unique(p, axis=0)
        rk = rank_of(p[:, 1] >> np.uint64(32))
        for g in np.unique(p[(rk == 0), 0]):
            found |= set(rk[p[:, 0] == g].tolist()) == {0, W - 1}
    assert found
    own = [s[2] for s in sc.steps["kstats"]]
    assert own[c.empty_owner] == 0 and sc.recv_counts[c.empty_owner].sum() == 0 and any(n % 64 for n in own)
    assert c.empty_owner in c.device_ranks and c.lonely[0] in c.device_ranks and {0, W - 1} <= set(c.device_ranks)
    whole = np.array(sc.steps["panel_counts"])
    win = [np.array(sc.steps["panel_counts_win%d" % i]) for i in range(5)]
    wl, wh = zip(*c.windows)
    assert (wl[0] == b[:-1]).all() and (wh[0] == b[1:]).all() and (win[0] == whole).all()                       # whole ranks
    assert (wl[1] == wh[1])[1::2].all() and win[1][:, 1::2].sum() == 0 and (win[1][:, 0::2] == whole[:, 0::2]).all()      # win_lo == win_hi for the odd ranks
    assert (wh[2] - wl[2] == 1).all() and (wl[2] == b[:-1]).all() and 0 < win[2].sum() < whole.sum()           # one row, a rank's first
    assert (wh[3] - wl[3] == 1).all() and (wh[3] == b[1:]).all() and 0 < win[3].sum() < whole.sum()            # one row, a rank's last
    lr, lrow = c.lonely
    assert wl[4][lr] == lrow and wh[4][lr] == lrow + 1 and b[lr] < lrow < b[lr + 1] - 1                        # a block in the middle of a rank ...
    assert win[4][:, lr].sum() == 0 and whole[:, lr].sum() > 0                                                  # ... that no column reaches
    assert (np.delete(win[4], lr, axis=1) == np.delete(whole, lr, axis=1)).all()
    # some column has the row just behind a one-row block and no row inside it: an off-by-one at the block's upper end changes the counts
    hit = False
    for r in range(W):
        p = np.concatenate(sc.steps["panel_send"][r])
        if not len(p):
            continue
        p = np.unique(p, axis=0)
        reads = (p[:, 1] >> np.uint64(32)).astype(np.int64)
        for d in range(W):
            behind = set(p[reads == wh[2][d], 0].tolist()) if wh[2][d] < b[d + 1] else set()
            inside = set(p[reads == wl[2][d], 0].tolist())
            hit |= bool(behind - inside)
    assert hit


# ---- the comparison rules reject what they must ---------------------------------------------------------------------------------------
def _segments(step, min_len=4):
    sc = dsc.script("short_reads")
    segs = [s.copy() for s in sc.steps[step][1]]
    assert sum(len(s) >= min_len for s in segs) >= 2
    return sc, segs


@pytest.mark.parametrize("step", ["send", "send8"])
def test_rules_reject_changed_and_misrouted_instance_records(step):
    sc, segs = _segments(step)
    want = sc.steps[step][1]
    dsc.assert_step_equal([s[::-1] for s in segs], want, step)                 # any order inside a destination's segment is fine
    bad = [s.copy() for s in segs]
    bad[0][3, -1] += np.uint64(1)                                              # one record's position changed
    with pytest.raises(AssertionError, match=step):
        dsc.assert_step_equal(bad, want, step)
    bad = [s.copy() for s in segs]
    bad[0][2], bad[1][2] = segs[1][2], segs[0][2]                              # two records of different destinations swapped
    with pytest.raises(AssertionError, match="destination 0"):
        dsc.assert_step_equal(bad, want, step)


def test_rules_reject_split_and_disordered_panel_columns():
    sc = dsc.script("short_reads")
    want = sc.steps["panel_send"][1]
    seg = want[0]
    g, n = np.unique(seg[:, 0], return_counts=True)
    assert len(g) > 3 and n.max() >= 3
    # whole columns in another order are fine
    cols = [seg[seg[:, 0] == x] for x in g]
    dsc.assert_step_equal([np.concatenate(cols[::-1])] + want[1:], want, "panel_send")
    big = int(np.argmax(n))
    a = cols[big]
    split = cols[:big] + [a[:1]] + cols[big + 1:] + [a[1:]] if big + 1 < len(cols) else [a[:1]] + cols[:big] + [a[1:]]
    with pytest.raises(AssertionError, match="more than one run"):             # a column split into two runs
        dsc.assert_step_equal([np.concatenate(split)] + want[1:], want, "panel_send")
    swapped = [c.copy() for c in cols]
    swapped[big][[0, 1]] = swapped[big][[1, 0]]
    with pytest.raises(AssertionError, match="order"):                         # a column with two entries swapped
        dsc.assert_step_equal([np.concatenate(swapped)] + want[1:], want, "panel_send")
    moved = [want[0][:-1], np.concatenate([want[1], want[0][-1:]])] + want[2:]
    with pytest.raises(AssertionError):                                        # a record in the wrong destination's segment
        dsc.assert_step_equal(moved, want, "panel_send")


def test_rules_compare_everything_else_exactly_and_in_order():
    sc = dsc.script("short_reads")
    u = sc.steps["unpack"][1]
    with pytest.raises(AssertionError, match="unpack"):
        dsc.assert_step_equal(u[::-1], u, "unpack")                            # unpacking is positional
    h = sc.steps["hist"][1].copy()
    h[7] += 1
    with pytest.raises(AssertionError, match="hist"):
        dsc.assert_step_equal(h, sc.steps["hist"][1], "hist")
    with pytest.raises(AssertionError, match="packed_fmt"):
        dsc.assert_step_equal(None, sc.fmt, "packed_fmt")


def test_numpy_packed_format_refuses_values_narrower_than_a_bin_index():
    """2k < 12 (stage_dist_packed_format: k2 < OWNER_BITS): None, not a shift by a negative count"""
    be = dist_sim.NumpyBackend(5, 2, 8)
    be.set_owner_ranges([1024, 4096])
    assert be.packed_format(2, [0, 1, 2], [30, 30]) is None
