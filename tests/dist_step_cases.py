"""Scripted worlds for the sharded build of A (elba_dist_* of include/elba_amd.h), CPU only: no torch.cuda, no DistributedOverlap.

A SCRIPT is the complete message log of one build: for every rank what it computes from its reads, what it sends to every other rank, what
it receives, and its rows of B.  It is computed with dist_sim.NumpyBackend instances alone, so a test sets owner ranges, read bounds,
record order and row windows directly, and ONE device context can then play one rank of a 64-rank world while the script plays the other 63:

    build_script(case)            -> Script: steps[name][rank] = what rank `rank` returns at step `name`, and the inputs of every step
    replay(backend, script, r)    -> drives any backend with HipBackend's interface through rank r's calls in order, feeding the script's
                                     inputs at each step; returns {step: output}; check(step, output) is called as soon as a step is done
    assert_step_equal(got, want, step)   the comparison rules (below)
    CASES / script(name)          the cases of tests/test_dist_steps_cpu.py (claims) and tests/test_gpu_dist_steps.py (device against script)

Comparison rules.  The device writes a destination's segment in no fixed order (blocks draw their places with atomics), so
  * instance records (steps send / send8): each destination's segment is compared as a sorted array of whole records;
  * panel records (steps panel_send*): a segment must consist of whole columns — all records of one global id adjacent, in (read, pos)
    order ("each column contiguous and internally ordered", elba_dist_set_panel) — and, the columns ordered by id, equal the script's;
  * everything else (histograms, counts, formats, unpacked records, statistics, reliable k-mers, rows of B): exact, in order.
"""
import functools

import numpy as np

import dist_sim
from elba_amd.distributed import kmer_words, owner_ranges_from_histogram
from oracle import pyoracle as po


# ---- reads ------------------------------------------------------------------------------------------------------------------------
def _dna(rng, n):
    return np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, int(n))].tobytes()


def _tile(genome, lens, step=997):
    """Read i = the substring of `genome` of length lens[i] at a start that walks the genome in steps of `step` (forward strand only: canonical
    k-mers make the strand irrelevant).  Coverage ~ sum(lens) / len(genome)."""
    return [genome[(i * step) % (len(genome) - int(n)):][:int(n)] for i, n in enumerate(lens)]


class Case:
    def __init__(self, name, k, lower, upper, seqs, bounds, upper_bins=None, windows=(), device_ranks=(0,)):
        self.name, self.k, self.lower, self.upper = name, k, lower, upper
        self.seqs = [bytes(s) for s in seqs]
        self.bounds = np.asarray(bounds, dtype=np.int64)
        self.W = len(self.bounds) - 1
        assert self.bounds[0] == 0 and self.bounds[-1] == len(self.seqs) and (np.diff(self.bounds) >= 0).all()
        self.upper_bins = None if upper_bins is None else np.asarray(upper_bins, dtype=np.uint32)      # None: from the summed histogram
        self.windows = [(np.asarray(a, dtype=np.int64), np.asarray(b, dtype=np.int64)) for a, b in windows]
        self.device_ranks = tuple(device_ranks)
        self.packed, self.off, self.lens = po.pack_reads(self.seqs)

    def shard(self, r):
        """reads [bounds[r], bounds[r+1]) in DnaBuffer layout with 16 guard bytes, and the first global read"""
        lo, hi = int(self.bounds[r]), int(self.bounds[r + 1])
        b0 = int(self.off[lo]) if lo < len(self.off) else 0
        b1 = int(self.off[hi - 1]) + (int(self.lens[hi - 1]) + 3) // 4 if hi > lo else b0
        return np.concatenate([self.packed[b0:b1], np.zeros(16, np.uint8)]), (self.off[lo:hi] - np.uint64(b0)), self.lens[lo:hi], lo

    def inst_off(self, r):
        """instance offsets of rank r's reads (reads shorter than k: empty ranges)"""
        n = np.maximum(self.lens[int(self.bounds[r]):int(self.bounds[r + 1])].astype(np.int64) - self.k + 1, 0)
        return np.concatenate([[0], np.cumsum(n)]).astype(np.int64)


# ---- tensors <-> arrays -------------------------------------------------------------------------------------------------------------
def _t(be, a, width=None):
    a = np.ascontiguousarray(a, dtype=np.uint64)
    if width is not None:
        a = a.reshape(-1, width)
    return be.torch.from_numpy(a.view(np.int64).copy()).to(be.dev)


def _n(t):
    return t.detach().cpu().numpy().view(np.uint64).copy()


def _excl(c):
    c = np.asarray(c, dtype=np.int64)
    return np.concatenate([[0], np.cumsum(c)[:-1]]).astype(np.int64)


def _split(a, counts):
    return [a[int(s):int(s + n)] for s, n in zip(_excl(counts), counts)]


def round_index(rc, rounds):
    """The chunked exchange of DistributedOverlap._exchange_packed_chunked: round t carries records [c * t // rounds, c * (t + 1) // rounds) of
    every peer's c.  -> per round (indices into the peer-major receive buffer, per-peer counts)."""
    rc = np.asarray(rc, dtype=np.int64)
    off = _excl(rc)
    out = []
    for t in range(rounds):
        lo, hi = rc * t // rounds, rc * (t + 1) // rounds
        out.append((np.concatenate([np.arange(off[p] + lo[p], off[p] + hi[p]) for p in range(len(rc))] + [np.zeros(0, np.int64)]).astype(np.int64), hi - lo))
    return out


STAT_FIELDS = ("instances", "distinct", "reliable", "entries")
SHUFFLE_SEED = 20240607


# ---- one rank's calls, in order -------------------------------------------------------------------------------------------------------
def replay(be, sc, r, check=None, record_order=None):
    """Rank r of script `sc` on backend `be`.  Inputs that come from other ranks (owner ranges, received records, id base, all owners'
    reliable k-mers, the received panel) are the script's; everything the rank computes itself is returned, step by step.
    record_order: a permutation of the received 16/24/32-byte records applied before count_records (the records arrive in no particular order)."""
    c = sc.case
    W, kw = c.W, kmer_words(c.k)
    out = {}

    def emit(step, value):
        out[step] = value
        if check is not None:
            check(step, value)

    sp, so, sl, first = c.shard(r)
    be.set_reads(sp, so, sl, first)
    emit("hist", np.asarray(be.value_histogram(), dtype=np.int64))
    if W > 1:
        be.set_owner_ranges(sc.upper_bins)
    oc = np.asarray(be.count_owners(W), dtype=np.int64)
    emit("owner_counts", oc)
    send = be.empty_records(int(oc.sum()), kw + 1)
    be.fill_send(W, send, _excl(oc))
    emit("send", _split(_n(send), oc))
    fmt = be.packed_format(W, c.bounds, c.lens) if kw == 1 else None
    emit("packed_fmt", None if fmt is None else (int(fmt[0]), int(fmt[1])))
    rc = np.asarray(sc.recv_counts[r], dtype=np.int64)
    if fmt is not None:
        send8 = be.empty_records(int(oc.sum()), 1)
        be.fill_send_packed(W, send8, _excl(oc))
        emit("send8", _split(_n(send8).reshape(-1, 1), oc))
        emit("unpack", _n(be.unpack_records(W, r, _t(be, sc.recv8[r], 1), rc)).reshape(-1, 2))
        recv = be.empty_records(int(rc.sum()), 2)
        at = 0
        for idx, counts in round_index(rc, 2):
            be.unpack_records(W, r, _t(be, sc.recv8[r][idx], 1), counts, out=recv[at:at + len(idx)])
            at += len(idx)
        emit("unpack_rounds", _n(recv).reshape(-1, 2))
    rec16 = sc.recv16[r] if record_order is None else sc.recv16[r][np.asarray(record_order)]
    rec = _t(be, rec16, kw + 1)                       # borrowed by the library until set_global_kmers has returned: alive to the end of this function
    st = be.count_records(rec)
    emit("kstats", tuple(int(st[f]) for f in STAT_FIELDS))
    emit("rel", _n(be.reliable_kmers(int(st["reliable"]))).reshape(-1, kw))
    # global ids, both ways on the same context: owners are value ranges, so rank in the union == base + index
    be.set_kmer_id_base(int(sc.base[r]), int(sc.n_total))
    pc = np.asarray(be.panel_counts(W, c.bounds), dtype=np.int64)
    emit("panel_counts", pc)
    ps = be.empty_records(int(pc.sum()), 2)
    be.panel_fill(W, c.bounds, ps, _excl(pc))
    emit("panel_send", _split(_n(ps).reshape(-1, 2), pc))
    be.set_global_kmers(_t(be, sc.all_kmers_shuffled).reshape(-1))
    pc = np.asarray(be.panel_counts(W, c.bounds), dtype=np.int64)
    emit("panel_counts_global", pc)
    ps = be.empty_records(int(pc.sum()), 2)
    be.panel_fill(W, c.bounds, ps, _excl(pc))
    emit("panel_send_global", _split(_n(ps).reshape(-1, 2), pc))
    for i, (wl, wh) in enumerate(c.windows):
        pc = np.asarray(be.panel_counts_win(W, c.bounds, wl, wh), dtype=np.int64)
        emit("panel_counts_win%d" % i, pc)
        ps = be.empty_records(int(pc.sum()), 2)
        be.panel_fill_win(W, c.bounds, wl, wh, ps, _excl(pc))
        emit("panel_send_win%d" % i, _split(_n(ps).reshape(-1, 2), pc))
    # the panel this rank receives -> its rows of B: no mirror exchange, no inline partners
    if hasattr(be, "set_option"):
        be.set_option("panel_inline", 0)
    lo, hi = int(c.bounds[r]), int(c.bounds[r + 1])
    be.set_panel(_t(be, sc.panel_in[r], 2), int(c.bounds[-1]), int(sc.n_total), lo, hi)
    be.create_seed_matrix()
    B = be.export_csr(lo, hi)
    emit("rows", dict(rowptr=np.asarray(B["rowptr"], dtype=np.int64), col=np.asarray(B["col"], dtype=np.int64), val=np.asarray(B["val"])))
    del rec
    return out


class Script:
    def __init__(self, case):
        self.case = case
        self.steps = {}


def build_script(case):
    """Every rank's log, with NumpyBackend alone.  Pass 1: what each rank makes of its reads; pass 2: the owners; pass 3: the panels."""
    c = case
    W, kw = c.W, kmer_words(c.k)
    sc = Script(c)
    S = sc.steps
    bes = [dist_sim.NumpyBackend(c.k, c.lower, c.upper) for _ in range(W)]
    for r, be in enumerate(bes):
        sp, so, sl, first = c.shard(r)
        be.set_reads(sp, so, sl, first)
    S["hist"] = [be.value_histogram() for be in bes]
    sc.upper_bins = c.upper_bins if c.upper_bins is not None else owner_ranges_from_histogram(np.sum(S["hist"], axis=0), W)
    if W > 1:
        for be in bes:
            be.set_owner_ranges(sc.upper_bins)
    S["owner_counts"] = [be.count_owners(W) for be in bes]
    S["send"], S["packed_fmt"], S["send8"] = [], [], []
    for r, be in enumerate(bes):
        oc = S["owner_counts"][r]
        send = be.empty_records(int(oc.sum()), kw + 1)
        be.fill_send(W, send, _excl(oc))
        S["send"].append(_split(_n(send), oc))
        fmt = be.packed_format(W, c.bounds, c.lens) if kw == 1 else None
        S["packed_fmt"].append(None if fmt is None else (int(fmt[0]), int(fmt[1])))
        if fmt is not None:
            s8 = be.empty_records(int(oc.sum()), 1)
            be.fill_send_packed(W, s8, _excl(oc))
            S["send8"].append(_split(_n(s8).reshape(-1, 1), oc))
    assert all(f == S["packed_fmt"][0] for f in S["packed_fmt"])               # "the same on every rank"
    sc.fmt = S["packed_fmt"][0]
    sc.recv_counts = [np.array([S["owner_counts"][s][r] for s in range(W)], dtype=np.int64) for r in range(W)]
    sc.recv16 = [np.concatenate([S["send"][s][r] for s in range(W)]) for r in range(W)]
    if sc.fmt is not None:
        sc.recv8 = [np.concatenate([S["send8"][s][r] for s in range(W)]).reshape(-1) for r in range(W)]
        S["unpack"] = [_n(bes[r].unpack_records(W, r, _t(bes[r], sc.recv8[r], 1), sc.recv_counts[r])).reshape(-1, 2) for r in range(W)]
        for r in range(W):
            assert np.array_equal(S["unpack"][r], sc.recv16[r]), "the two wire formats of the script disagree"
        S["unpack_rounds"] = [sc.recv16[r][np.concatenate([idx for idx, _ in round_index(sc.recv_counts[r], 2)])] for r in range(W)]
    else:
        del S["send8"]
    S["kstats"], S["rel"] = [], []
    for r, be in enumerate(bes):
        st = be.count_records(_t(be, sc.recv16[r], kw + 1))
        S["kstats"].append(tuple(int(st[f]) for f in STAT_FIELDS))
        S["rel"].append(_n(be.reliable_kmers(st["reliable"])).reshape(-1, kw))
    ns = [len(x) for x in S["rel"]]
    sc.n_total = int(sum(ns))
    sc.base = _excl(ns)
    allk = np.concatenate(S["rel"])
    sc.all_kmers_shuffled = allk[np.random.default_rng(SHUFFLE_SEED).permutation(len(allk))]
    S["gid"] = []
    for r, be in enumerate(bes):
        be.set_kmer_id_base(int(sc.base[r]), sc.n_total)
        S["gid"].append(be.gid.copy())
    S["panel_counts"], S["panel_send"] = [], []
    for i in range(len(c.windows)):
        S["panel_counts_win%d" % i], S["panel_send_win%d" % i] = [], []
    for r, be in enumerate(bes):
        pc = be.panel_counts(W, c.bounds)
        ps = be.empty_records(int(pc.sum()), 2)
        be.panel_fill(W, c.bounds, ps, _excl(pc))
        S["panel_counts"].append(pc); S["panel_send"].append(_split(_n(ps).reshape(-1, 2), pc))
        for i, (wl, wh) in enumerate(c.windows):
            pc = be.panel_counts_win(W, c.bounds, wl, wh)
            ps = be.empty_records(int(pc.sum()), 2)
            be.panel_fill_win(W, c.bounds, wl, wh, ps, _excl(pc))
            S["panel_counts_win%d" % i].append(pc); S["panel_send_win%d" % i].append(_split(_n(ps).reshape(-1, 2), pc))
    S["panel_counts_global"], S["panel_send_global"] = S["panel_counts"], S["panel_send"]
    sc.panel_in = [np.concatenate([S["panel_send"][s][r] for s in range(W)]) for r in range(W)]
    S["rows"] = []
    for r, be in enumerate(bes):
        lo, hi = int(c.bounds[r]), int(c.bounds[r + 1])
        be.set_panel(_t(be, sc.panel_in[r], 2), int(c.bounds[-1]), sc.n_total, lo, hi)
        be.create_seed_matrix()
        B = be.export_csr(lo, hi)
        S["rows"].append(dict(rowptr=np.asarray(B["rowptr"], dtype=np.int64), col=np.asarray(B["col"], dtype=np.int64), val=np.asarray(B["val"])))
    return sc


# ---- comparison rules ---------------------------------------------------------------------------------------------------------------
def _sorted_records(a):
    a = np.asarray(a, dtype=np.uint64)
    if len(a) == 0:
        return a
    a = a.reshape(len(a), -1)
    return a[np.lexsort([a[:, w] for w in range(a.shape[1] - 1, -1, -1)])]


def _whole_columns(seg, step, d):
    """panel records of one destination: whole columns, each contiguous and in (read, pos) order -> the columns ordered by id"""
    seg = np.asarray(seg, dtype=np.uint64).reshape(-1, 2)
    if len(seg) == 0:
        return seg
    g = seg[:, 0]
    starts = np.flatnonzero(np.concatenate([[True], g[1:] != g[:-1]]))
    assert len(np.unique(g[starts])) == len(starts), "%s: destination %d: a column comes in more than one run" % (step, d)
    same = g[1:] == g[:-1]
    assert (seg[1:, 1][same] > seg[:-1, 1][same]).all(), "%s: destination %d: a column is not in (read, pos) order" % (step, d)
    return seg[np.argsort(g, kind="stable")]


def assert_step_equal(got, want, step, where=""):
    """where: put in front of the step's name in every message (case and rank)"""
    kind, step = step, where + step
    if kind.startswith("send"):                                  # instance records, 8 / 16 / 24 / 32 bytes: per destination, as sorted whole records
        assert len(got) == len(want), "%s: %d destinations, want %d" % (step, len(got), len(want))
        for d, (g, w) in enumerate(zip(got, want)):
            assert np.shape(g) == np.shape(w), "%s: destination %d: %s records, want %s" % (step, d, np.shape(g), np.shape(w))
            assert np.array_equal(_sorted_records(g), _sorted_records(w)), "%s: destination %d: the records differ" % (step, d)
    elif kind.startswith("panel_send"):
        assert len(got) == len(want), "%s: %d destinations, want %d" % (step, len(got), len(want))
        for d, (g, w) in enumerate(zip(got, want)):
            assert np.shape(g) == np.shape(w), "%s: destination %d: %s records, want %s" % (step, d, np.shape(g), np.shape(w))
            assert np.array_equal(_whole_columns(g, step, d), _whole_columns(w, step + " (script)", d)), "%s: destination %d: the columns differ" % (step, d)
    elif kind == "rows":
        for f in ("rowptr", "col", "val"):
            assert len(got[f]) == len(want[f]) and (got[f] == want[f]).all(), "%s: %s differs" % (step, f)
    elif want is None or isinstance(want, tuple):
        assert got == want, "%s: %r, want %r" % (step, got, want)
    else:
        g, w = np.asarray(got), np.asarray(want)
        assert g.shape == w.shape and np.array_equal(g, w), "%s: differs (first at %s)" % (step, np.argwhere(g != w)[:1].tolist() if g.shape == w.shape else (g.shape, w.shape))


def checker(sc, r):
    """check= of replay: every step against the script's rank r, as soon as it is there"""
    return lambda step, got: assert_step_equal(got, sc.steps[step][r], step, "%s, rank %d: " % (sc.case.name, r))


# ---- the cases ------------------------------------------------------------------------------------------------------------------------
K17 = 17


def _even_bounds(n, W):
    return (np.arange(W + 1, dtype=np.int64) * n) // W


def _long_lens(rng, n, lo=560, hi=720):
    return rng.integers(lo, hi, n).tolist()


def case_short_reads():
    """reads of 1, k-1, k, k+1 bases among long ones: at the start of shard 0, as a run in the middle of shard 1 (the first instance behind
    it at a wave's g0), a second run in the middle of a wave, and at the end of shard 2"""
    k, rng = K17, np.random.default_rng(11)
    s0 = [1, k - 1, k, k + 1] + _long_lens(rng, 16)
    s1 = [300 + k - 1, 724 + k - 1, 512 + k - 1, 512 + k - 1, 1, k - 1, 7, k, k + 1, 600, 3, k - 1] + _long_lens(rng, 14)
    s2 = _long_lens(rng, 16) + [k + 1, k, 1, k - 1]
    lens = s0 + s1 + s2
    return Case("short_reads", k, 2, 8, _tile(_dna(rng, 6500), lens), [0, len(s0), len(s0) + len(s1), len(lens)], device_ranks=(0, 1, 2))


def case_empty_ranks():
    """bounds with equal neighbours: ranks 0, 2 and 4 have no reads, rank 3's reads are all shorter than k — every instance comes from rank 1,
    every rank is an owner all the same"""
    k, rng = K17, np.random.default_rng(12)
    s1 = _long_lens(rng, 40)
    s3 = [1, k - 1, 5, k - 1, 9]
    lens = s1 + s3
    n1, n = len(s1), len(lens)
    return Case("empty_ranks", k, 2, 8, _tile(_dna(rng, 5000), lens), [0, 0, n1, n1, n, n], device_ranks=(0, 1, 2, 3, 4))


def _reads_64(seed, per_rank=5, rlen=150, cover=5):
    rng = np.random.default_rng(seed)
    lens = rng.integers(rlen - 20, rlen + 20, 64 * per_rank).tolist()
    return rng, lens, _tile(_dna(rng, sum(lens) // cover), lens, step=613)


def case_owners_64(hand):
    """64 owners: ranges from the histogram, or set by hand with repeated boundaries (owner 0, owner 31 and owner 63 own nothing)"""
    rng, lens, seqs = _reads_64(13)
    c = Case("owners_64_hand" if hand else "owners_64_hist", K17, 2, 8, seqs, _even_bounds(len(lens), 64), device_ranks=(0, 1, 31, 32, 62, 63) if hand else (0, 31, 62, 63))
    if hand:
        h = np.sum([np.bincount((po_first_words(c, r) >> np.uint64(52)).astype(np.int64), minlength=4096) for r in range(64)], axis=0)
        u = owner_ranges_from_histogram(h, 64).astype(np.int64)
        u[0] = 0; u[31] = u[30]; u[62] = 4096; u[63] = 4096
        c.upper_bins = u.astype(np.uint32)
    return c


def po_first_words(case, r):
    """first words of the canonical k-mer instances of rank r's reads (the oracle's enumerator)"""
    be = dist_sim.NumpyBackend(case.k, case.lower, case.upper)
    be.set_reads(*case.shard(r))
    return be._first_word()


def _exact_instances(k, per_rank, nranks, nreads):
    """`nreads` reads per rank whose instances add up to exactly `per_rank` on every rank"""
    base = per_rank // nreads
    n = [base] * (nreads - 1) + [per_rank - base * (nreads - 1)]
    return [x + k - 1 for _ in range(nranks) for x in n]


def case_packed_limit(which):
    """the format decision at its edge (value bits + index bits <= 64), owner ranges set by hand"""
    rng = np.random.default_rng(14)
    if which in ("k27_fits", "k27_over"):                     # 2 equal owners: 53 value bits; 2048 instances per rank: 11 index bits, 2049: 12
        k, W = 27, 2
        lens = _exact_instances(k, 2048, W, 8)
        seqs = _tile(_dna(rng, 1700), lens, step=211)
        if which == "k27_over":
            seqs[-1] = seqs[-1] + b"G"
        return Case("packed_" + which, k, 2, 8, seqs, _even_bounds(len(lens), W), upper_bins=[2048, 4096], device_ranks=(0, 1))
    if which in ("k31_fits", "k31_over"):                     # 64 owners of 64 bins: 56 value bits; 256 instances per rank: 8 index bits, 257: 9
        k, W = 31, 64
        lens = _exact_instances(k, 256, W, 2)
        seqs = _tile(_dna(rng, 4000), lens, step=61)
        if which == "k31_over":
            seqs[0] = b"C" + seqs[0]
        return Case("packed_" + which, k, 2, 8, seqs, _even_bounds(len(lens), W), upper_bins=64 * (np.arange(64) + 1), device_ranks=(0, 63) if which == "k31_fits" else (0,))
    if which == "k7":                                          # one owner: 14 value bits, the index bits of the instances
        lens = rng.integers(130, 170, 40).tolist()
        return Case("packed_k7", 7, 2, 8, _tile(_dna(rng, 6000), lens), [0, len(lens)], device_ranks=(0,))
    assert which == "k5"                                       # 2k < 12: a value has fewer bits than a bin index: never packed
    lens = [28, 31, 33, 30, 29, 32]
    return Case("packed_k5", 5, 2, 8, _tile(_dna(rng, 400), lens, step=37), [0, 3, 6], upper_bins=[1024, 4096], device_ranks=(0, 1))


def case_multiword(k):
    """two / three words per k-mer; a planted repeat whose two copies differ only past base 32 / 64: two reliable k-mers of one owner that
    share their first word (first two words)"""
    rng = np.random.default_rng(15 + k)
    W = 3 if k == 33 else 2
    lens = rng.integers(280, 360, 60 if k == 33 else 50).tolist()
    g = bytearray(_dna(rng, sum(lens) // 5))
    stem = b"AA" + _dna(rng, k - 3)                            # k - 1 bases starting with A: stem + A and stem + C are both smaller than their twins (T..., G...)
    g[1000:1000 + k] = stem + b"A"
    g[2000:2000 + k] = stem + b"C"
    c = Case("multiword_%d" % k, k, 2, 12, _tile(bytes(g), lens, step=97), _even_bounds(len(lens), W), device_ranks=tuple(range(W)))
    c.stem = stem
    return c


def case_count_edges(lower, upper):
    """the owner's exact count at its thresholds: unit c (40 unique bases) occurs in exactly c reads, c = 1 .. 41; unit D twice in read 0 and
    once in read 1"""
    rng = np.random.default_rng(16)
    nreads = 100
    units = {cnt: _dna(rng, 40) for cnt in range(1, 42)}
    reads = [bytearray() for _ in range(nreads)]
    at = 0
    for cnt in range(1, 42):
        for _ in range(cnt):
            reads[at % nreads] += units[cnt]
            at += 1
    D = _dna(rng, 40)
    reads[0] = D + reads[0] + D
    reads[1] = reads[1] + D
    c = Case("count_edges_%d_%d" % (lower, upper), K17, lower, upper, [bytes(x) for x in reads], _even_bounds(nreads, 2), device_ranks=(0, 1))
    c.unit_D = D
    return c


def window_sets(bounds, lonely):
    """Row blocks (win_lo[W], win_hi[W]): whole ranks; nothing for the odd ranks; the first row of every rank; the last row of every rank; and
    `lonely` = (rank, row): that rank's block is the one row no column reaches, the others keep theirs whole."""
    b = np.asarray(bounds, dtype=np.int64)
    lo, hi = b[:-1].copy(), b[1:].copy()
    odd = (np.arange(len(lo)) & 1) == 1
    sets = [(lo, hi), (lo, np.where(odd, lo, hi)), (lo, np.minimum(lo + 1, hi)), (np.maximum(hi - 1, lo), hi)]
    wl, wh = lo.copy(), hi.copy()
    wl[lonely[0]], wh[lonely[0]] = lonely[1], lonely[1] + 1
    return sets + [(wl, wh)]


def case_panel_windows(W):
    """destinations and row blocks: a column shared by the first and the last read only (ranks 0 and W - 1), an owner without reliable k-mers,
    a read that shares no k-mer with any other"""
    if W == 64:
        rng, lens, seqs = _reads_64(17)
    else:
        rng = np.random.default_rng(18)
        lens = _long_lens(rng, 60)
        seqs = _tile(_dna(rng, sum(lens) // 5), lens)
    X = _dna(rng, 40)
    seqs[0] = seqs[0][:50] + X + seqs[0][90:]
    seqs[-1] = seqs[-1][:50] + X + seqs[-1][90:]
    bounds = _even_bounds(len(seqs), W)
    lonely_rank = 10 if W == 64 else 1
    lonely_row = int(bounds[lonely_rank]) + 2
    seqs[lonely_row] = _dna(rng, len(seqs[lonely_row]))
    c = Case("panel_windows_%d" % W, K17, 2, 8, seqs, bounds, windows=window_sets(bounds, (lonely_rank, lonely_row)),
             device_ranks=(0, 5, 10, 32, 63) if W == 64 else (0, 1, 2))
    h = np.sum([np.bincount((po_first_words(c, r) >> np.uint64(52)).astype(np.int64), minlength=4096) for r in range(W)], axis=0)
    u = owner_ranges_from_histogram(h, W).astype(np.int64)
    empty_owner = 5 if W == 64 else 1
    u[empty_owner] = u[empty_owner - 1]                        # this owner's range is empty: own_N == 0
    c.upper_bins = u.astype(np.uint32)
    c.unit_X, c.lonely, c.empty_owner = X, (lonely_rank, lonely_row), empty_owner
    return c


CASES = {
    "short_reads": case_short_reads,
    "empty_ranks": case_empty_ranks,
    "owners_64_hist": lambda: case_owners_64(False),
    "owners_64_hand": lambda: case_owners_64(True),
    "packed_k27_fits": lambda: case_packed_limit("k27_fits"),
    "packed_k27_over": lambda: case_packed_limit("k27_over"),
    "packed_k31_fits": lambda: case_packed_limit("k31_fits"),
    "packed_k31_over": lambda: case_packed_limit("k31_over"),
    "packed_k7": lambda: case_packed_limit("k7"),
    "packed_k5": lambda: case_packed_limit("k5"),
    "multiword_33": lambda: case_multiword(33),
    "multiword_65": lambda: case_multiword(65),
    "count_edges_2_4": lambda: case_count_edges(2, 4),
    "count_edges_3_3": lambda: case_count_edges(3, 3),
    "count_edges_2_40": lambda: case_count_edges(2, 40),
    "panel_windows_64": lambda: case_panel_windows(64),
    "panel_windows_3": lambda: case_panel_windows(3),
}


@functools.lru_cache(maxsize=None)
def script(name):
    """the script of a case, computed once per process and shared (treat it as read-only)"""
    return build_script(CASES[name]())


def record_orders(n):
    """the three arrival orders of count_edges: as sent, reversed, shuffled with a fixed seed"""
    return dict(sent=np.arange(n), reversed=np.arange(n)[::-1].copy(), shuffled=np.random.default_rng(SHUFFLE_SEED + 1).permutation(n))
