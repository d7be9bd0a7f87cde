"""Case builders for the boundary tests of the read pileup (pileup.hip): pair lists aimed at one branch of one kernel each, with what
every case claims about itself.  No GPU and no pytest here: test_pileup_cases_cpu.py holds every claim against the restatement
(pileup_util.py) before test_gpu_pileup_edges.py spends GPU time on a case.

A Case carries lens, rows, cols, vals, its pileup settings `cfgs` (the claims speak of cfgs[0]) and `claims`:
  E          credited endpoints (2 x credited intervals)
  key_bits   mb + pb + 1 by stage_read_pileup's formula; read_top / pos_top: an endpoint with bit mb - 1 of the read field / bit pb - 1 of
             the position field set
  max_depth, segs {read: [(start, depth), ...]}, profile {read: per-base depth}, trim {read: (beg, end)}, flags {read: flags},
  runs {read: runs of depth >= min_depth}, curbases (the largest running sum of one run), stats {name: value}
`reads` lists the reads whose profile and trimmed interval the CPU tests recompute base by base (None: every read)."""
import functools

import numpy as np

import pileup_util as pu
import string_graph_util as sgu
import trim_util as tu
from elba_amd.capi import OVERLAP_DTYPE

BASE = dict(mode=1, margin=0, min_depth=1, min_run=1, trim_len=0)
INT_MAX = 2**31 - 1


class Case:
    def __init__(self, name, lens, rows, cols, vals, cfgs, reads=None, **claims):
        self.name = name
        self.lens = np.ascontiguousarray(lens, dtype=np.int64)
        self.rows = np.ascontiguousarray(rows, dtype=np.int64); self.cols = np.ascontiguousarray(cols, dtype=np.int64)
        self.vals = np.ascontiguousarray(vals, dtype=OVERLAP_DTYPE)
        self.cfgs = [dict(BASE, **c) for c in cfgs]
        self.reads = reads
        self.claims = claims

    def __repr__(self):
        return self.name

    @property
    def args(self):
        return self.lens, self.rows, self.cols, self.vals


_pileup = pu.pileup
_memo = {}


def pileup_memo(lens, rows, cols, vals, **cfg):
    """pileup_util.pileup, computed once per (arrays of a cached case, settings): the cases' arrays are never written to."""
    key = (id(lens), id(rows), id(cols), id(vals), tuple(sorted(cfg.items())))
    if key not in _memo:
        _memo[key] = (_pileup(lens, rows, cols, vals, **cfg), (lens, rows, cols, vals))      # (the arrays stay alive: ids stay theirs)
    return _memo[key][0]


def reference(case, cfg):
    return pileup_memo(*case.args, **cfg)


def key_bits(lens):
    """(mb, pb) of stage_read_pileup: read ids 0 .. M and positions 0 .. the longest read."""
    M = len(lens)
    mx = int(np.max(lens)) if M else 0
    mb = pb = 1
    while (1 << mb) < M + 1:
        mb += 1
    while (1 << pb) < mx + 1:
        pb += 1
    return mb, pb


def both_modes(**cfg):
    return [dict(cfg, mode=1), dict(cfg, mode=0)]


def _hand(name, lens, intervals, cfgs=None, **claims):
    """The pair list that credits exactly the given (read, beg, end) intervals (trim_util.overlaps_for), accepted in both modes."""
    rows, cols, vals = tu.overlaps_for(len(lens), intervals)
    vals["passed"] = 1
    claims.setdefault("E", 2 * len(intervals))
    return Case(name, lens, rows, cols, vals, cfgs if cfgs is not None else both_modes(), **claims)


def intervals_of_profile(r, p):
    """Intervals on read r whose pileup is the per-base depth p: one per maximal stretch of depth >= d, for every d."""
    p = np.asarray(p, dtype=np.int64)
    out = []
    for d in range(1, int(p.max()) + 1 if len(p) else 1):
        m = np.diff(np.concatenate([[0], (p >= d).astype(np.int8), [0]]))
        out += [(r, int(a), int(b)) for a, b in zip(np.flatnonzero(m == 1), np.flatnonzero(m == -1))]
    return out


def _profiles(name, profiles, cfgs, **claims):
    """Read i + 1 gets profiles[i]; read 0 and enough reads behind them (3 bases each) serve as partners."""
    ivs = [iv for i, p in enumerate(profiles) for iv in intervals_of_profile(i + 1, p)]
    most = max(sum(1 for iv in ivs if iv[0] == i + 1) for i in range(len(profiles)))
    M = max(len(profiles) + 2, most + 2)
    lens = [3] * M
    for i, p in enumerate(profiles):
        lens[i + 1] = len(p)
    return _hand(name, lens, ivs, cfgs, profile={i + 1: list(p) for i, p in enumerate(profiles)}, **claims)


# ---- keys wider than 32 bits ------------------------------------------------------------------------------------------------------------

def _wide(name, M, long_reads, per_long, seed, bits):
    """M reads of 0 .. 8 bases except long_reads {id: bases}; per_long pairs on every long read with intervals in its upper half, a quarter
    of them ending exactly at len; 300 pairs among the short reads.  passed and score are drawn independently: the two modes differ."""
    rng = np.random.default_rng(seed)
    lens = rng.integers(0, 9, M).astype(np.int64)
    for v, L in long_reads.items():
        lens[v] = L
    pairs = set()
    for v in long_reads:
        others = np.setdiff1d(np.arange(M), [v])
        for t in rng.choice(others, size=min(per_long, len(others)), replace=False):
            pairs.add((min(v, int(t)), max(v, int(t))))
    while len(pairs) < len(long_reads) * min(per_long, M - 1) + 300:
        a, b = (int(x) for x in rng.integers(0, M, 2))
        if a != b:
            pairs.add((min(a, b), max(a, b)))
    pairs = sorted(pairs)
    rows = np.array([p[0] for p in pairs], np.int64); cols = np.array([p[1] for p in pairs], np.int64)
    vals = np.zeros(len(pairs), OVERLAP_DTYPE)
    for f0, f1, who in (("begQ", "endQ", rows), ("begT", "endT", cols)):
        L = lens[who]
        lo = np.where(L > 8, L // 2, 0)
        x = np.sort(np.stack([rng.integers(lo, L + 1), rng.integers(lo, L + 1)], 1), 1)
        at_end = (L > 8) & (rng.integers(0, 4, len(L)) == 0)
        x[at_end, 1] = L[at_end]
        vals[f0], vals[f1] = x[:, 0], x[:, 1]
    vals["passed"] = rng.integers(0, 2, len(pairs))
    vals["score"] = rng.integers(-1, 50, len(pairs))
    cfgs = [dict(mode=1, margin=0, min_depth=2, min_run=50, trim_len=1000), dict(mode=0, margin=3, min_depth=1, min_run=1, trim_len=0)]
    return Case(name, lens, rows, cols, vals, cfgs, reads=sorted(long_reads), key_bits=bits, read_top=True, pos_top=True)


@functools.lru_cache(maxsize=None)
def wide_key_cases():
    return (_wide("bits32_M1025_len2p19", 1025, {1024: 2**19 + 1000}, 1000, 31, 32),         # mb 11, pb 20: four sort passes
            _wide("bits34_M2049_len2p20", 2049, {2048: 2**20}, 2048, 32, 34),                # mb 12, pb 21: five
            _wide("bits35_M65537_len2p16", 65537, {65536: 65536, 0: 32768}, 2500, 33, 35))   # mb 17, pb 17: five


# ---- degenerate launches ----------------------------------------------------------------------------------------------------------------

def _random_list(seed, M, n, lo=100, hi=500):
    rng = np.random.default_rng(seed)
    lens = rng.integers(lo, hi, M).astype(np.int64)
    pairs = set()
    while len(pairs) < n:
        a, b = (int(x) for x in rng.integers(0, M, 2))
        if a != b:
            pairs.add((min(a, b), max(a, b)))
    pairs = sorted(pairs)
    rows = np.array([p[0] for p in pairs], np.int64); cols = np.array([p[1] for p in pairs], np.int64)
    vals = np.zeros(n, OVERLAP_DTYPE)
    for f0, f1, who in (("begQ", "endQ", rows), ("begT", "endT", cols)):
        L = lens[who]
        x = np.sort(np.stack([rng.integers(0, L + 1), rng.integers(0, L + 1)], 1), 1)
        vals[f0], vals[f1] = x[:, 0], x[:, 1]
    vals["passed"] = 1; vals["score"] = 7
    return lens, rows, cols, vals


@functools.lru_cache(maxsize=None)
def degenerate_cases():
    out = []
    lens, rows, cols, vals = _random_list(61, 40, 120)
    v = vals.copy(); v["passed"] = 0
    out.append(Case("none_passed_mode0", lens, rows, cols, v, [dict(mode=0)], E=0, stats=dict(pairs=0, intervals=0, segments=40)))
    v = vals.copy(); v["score"] = np.where(np.arange(120) % 2, 0, -5)
    out.append(Case("none_scored_mode1", lens, rows, cols, v, [dict(mode=1)], E=0, stats=dict(pairs=0, intervals=0, segments=40)))
    out.append(Case("margin_int_max", lens, rows, cols, vals, both_modes(margin=INT_MAX), E=0, stats=dict(pairs=120, intervals=0, segments=40)))
    longest = int(max((vals["endQ"] - vals["begQ"]).max(), (vals["endT"] - vals["begT"]).max()))
    half = (longest + 1) // 2
    out.append(Case("margin_half_longest", lens, rows, cols, vals, both_modes(margin=half) + [dict(margin=half - 1)], E=0, longest=longest,
                    stats=dict(pairs=120, intervals=0, segments=40)))
    rng = np.random.default_rng(62)
    for M in (1, 255, 256, 257):
        ln = rng.integers(0, 20, M).astype(np.int64)
        ln[0] = 5 if M == 1 else 0
        out.append(Case("n0_M%d" % M, ln, [], [], np.zeros(0, OVERLAP_DTYPE), both_modes(trim_len=3), E=0,
                        stats=dict(pairs=0, intervals=0, segments=int((ln > 0).sum()))))
    out.append(Case("M0", [], [], [], np.zeros(0, OVERLAP_DTYPE), both_modes(), E=0, stats=dict(nreads=0, pairs=0, intervals=0, segments=0)))
    return tuple(out)


# ---- block edges of the E + 1 slots and of the max(E, M) + 1 lanes ------------------------------------------------------------------------

def _edge(E, M):
    """E / 2 intervals, two per read, on reads spread over 0 .. M - 1; every read has 6 .. 10 bases."""
    nint = E // 2
    used = (nint + 1) // 2
    stride = max(1, M // used)
    lens = [6 + r % 5 for r in range(M)]
    ivs = []
    for i in range(nint):
        r = (i // 2) * stride
        ivs.append((r, i % 3, lens[r] - i % 2))
    return _hand("E%d_M%d" % (E, M), lens, ivs, both_modes(min_depth=2, min_run=4, trim_len=2), E=E)


@functools.lru_cache(maxsize=None)
def block_edge_cases():
    out = []
    for E in (2, 254, 256, 258, 510, 512, 514):
        for M in (E - 1, E, E + 1) + ((255, 256, 257) if E == 2 else ()):
            if M >= 2:                                                # (one read has no partner: E = 2 with M = 1 does not exist)
                out.append(_edge(E, M))
    return tuple(out)


# ---- the emission rules, on one read between reads without endpoints ----------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def emission_cases():
    out = []
    L, x, r = 50, 20, 2
    lens = [7, 3, L, 4, 9]
    for name, iv, segs in (("0_x", (0, x), [(0, 1), (x, 0)]), ("x_len", (x, L), [(0, 0), (x, 1)]), ("0_len", (0, L), [(0, 1)]),
                           ("last_base", (L - 1, L), [(0, 0), (L - 1, 1)]), ("first_base", (0, 1), [(0, 1), (1, 0)])):
        out.append(_hand("one_" + name, lens, [(r, iv[0], iv[1])], segs={r: segs, 1: [(0, 0)], 3: [(0, 0)]}))
    rng = np.random.default_rng(63)
    for k in (1, 64, 3000):
        # k intervals end at x and j start there: no boundary for j == k, one for j == k +- 1
        for j in (k, k - 1, k + 1):
            M = k + j + 4
            r = M // 2
            lens = rng.integers(0, 5, M); lens[r] = L
            segs = [(0, 0), (5, k)] + ([(x, j)] if j != k else []) + ([(L - 5, 0)] if j else [])
            out.append(_hand("mid_%d_ends_%d_starts" % (k, j), lens, [(r, 5, x)] * k + [(r, x, L - 5)] * j, segs={r: segs}, max_depth=max(k, j)))
        # position 0 can only hold starts (an end at 0 is an empty interval) and position len only ends
        M = k + 3
        r = M // 2
        lens = rng.integers(0, 5, M); lens[r] = L
        out.append(_hand("zero_%d_starts" % k, lens, [(r, 0, 30)] * k, segs={r: [(0, k), (30, 0)]}, max_depth=k))
        out.append(_hand("len_%d_ends" % k, lens, [(r, 10, L)] * k, segs={r: [(0, 0), (10, k)]}, max_depth=k))
    out.append(_hand("emptied_by_margin_between_kept", [40, 40, 40, 2], [(0, 0, 40), (1, 5, 9), (1, 10, 16), (2, 0, 40)], both_modes(margin=3), E=4,
                     segs={0: [(0, 0), (3, 1), (37, 0)], 1: [(0, 0)], 2: [(0, 0), (3, 1), (37, 0)]}))
    out.append(_hand("empty_reads_first_last_and_two_in_a_row", [0, 12, 0, 0, 9, 0], [(1, 2, 12), (4, 0, 5)],
                     segs={0: [], 1: [(0, 0), (2, 1)], 2: [], 3: [], 4: [(0, 1), (5, 0)], 5: []}))
    # 300 reads in no pair at all between the two reads of the only pair: their tokens sit back to back
    lens = rng.integers(0, 10, 303); lens[0] = 30; lens[301] = 25
    vals = np.zeros(1, OVERLAP_DTYPE)
    vals["begQ"], vals["endQ"], vals["begT"], vals["endT"], vals["passed"], vals["score"] = 3, 30, 0, 20, 1, 1
    out.append(Case("300_reads_without_pairs", lens, [0], [301], vals, both_modes(), E=4, segs={0: [(0, 0), (3, 1)], 301: [(0, 1), (20, 0)]}))
    return tuple(out)


# ---- the closed form of k_pu_reads --------------------------------------------------------------------------------------------------------

def _deep_run():
    """Depth 40 000 over 60 000 bases of read 0 and 40 001 over the last 100 of them: the average rises base by base through the tail, so the
    best run ends where curbases is 2.4e9 > 2^31 (a sum held in 32 bits would leave the best at the first eligible base)."""
    K, W, s = 40000, 60000, 3
    M = K + 3
    rng = np.random.default_rng(64)
    lens = rng.integers(0, 5, M).astype(np.int64); lens[0] = W + 7
    rows = np.zeros(K + 1, np.int64); cols = np.arange(1, K + 2, dtype=np.int64)
    vals = np.zeros(K + 1, OVERLAP_DTYPE)
    vals["begQ"] = s; vals["endQ"] = s + W
    vals["begQ"][K] = s + W - 100
    vals["passed"] = 1; vals["score"] = 1
    return Case("deep_run_curbases_over_2p31", lens, rows, cols, vals, [dict(trim_len=2500), dict(mode=0, trim_len=0, min_depth=40001)], reads=[0],
                E=2 * (K + 1), max_depth=K + 1, curbases=K * W + 100, trim={0: (s, s + W)}, runs={0: 1})


@functools.lru_cache(maxsize=None)
def trim_cases():
    out = []
    T, s = 20, 5
    cfgs = both_modes(trim_len=T)
    rising, falling = [], []
    for off in (-1, 0, 1):                                        # a segment boundary at s + T - 1, s + T, s + T + 1
        rising.append([0] * s + [2] * (T + off) + [3] * 10 + [0] * 3)
        falling.append([0] * s + [3] * (T + off) + [2] * 10 + [0] * 3)
    out.append(_profiles("boundary_at_start_plus_T_rising", rising, cfgs, trim={1: (s, s + T + 9), 2: (s, s + T + 10), 3: (s, s + T + 11)}))
    out.append(_profiles("boundary_at_start_plus_T_falling", falling, cfgs, trim={1: (s, s + T + 1), 2: (s, s + T + 1), 3: (s, s + T + 1)}))
    out.append(_profiles("run_ends_at_start_plus_T", [[0] * s + [2] * T + [0] * 4, [0] * s + [2] * (T + 1) + [0] * 4, [0] * s + [2] * T, [0] * s + [2] * (T + 1)], cfgs,
                         trim={1: (-1, -1), 2: (s, s + T + 1), 3: (-1, -1), 4: (s, s + T + 1)}))
    # the first run's average rises to its end: maxlen becomes L1 = 30; a later, deeper run wins only with more than L1 bases
    first = [0] * s + [1] * 10 + [2] * 20 + [0] * 3
    out.append(_profiles("second_run_against_raised_maxlen", [first + [5] * 30 + [0], first + [5] * 31 + [0], first + [5] * 29 + [0], first + [5] * 31], cfgs,
                         trim={1: (s, s + 30), 2: (s + 33, s + 64), 3: (s, s + 30), 4: (s + 33, s + 64)}))
    # 4a + 2b + 6b = 4 (a + 2b): the average is 4.0 again at the last base of the run and must not replace the best (strictly greater)
    tie = [0] * 2 + [4] * 30 + [2] * 10 + [6] * 10
    out.append(_profiles("average_ties", [tie + [0], tie, tie + [6, 0], [4] * 50], cfgs, trim={1: (2, 23), 2: (2, 23), 3: (2, 53), 4: (0, 21)}))
    p = [0] * 3 + [2] * 10 + [3] * 7 + [0] * 2
    out.append(_profiles("trim_len_range", [p], [dict(trim_len=t) for t in (0, 1, len(p) - 1, len(p), INT_MAX, 16, 17)],
                         trim={1: (3, 20)}))
    out.append(_deep_run())
    return tuple(out)


# ---- flags --------------------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def flag_cases():
    D, R = 3, 10
    profiles = [[0] * 2 + [D] * (R - 1) + [0] * 2,            # 1: a run of min_run - 1
                [0] * 2 + [D] * R + [0] * 2,                  # 2: of min_run
                [0] * 2 + [D] * (R + 1) + [0] * 2,            # 3: of min_run + 1
                [D - 1] * 30,                                 # 4: depth min_depth - 1 throughout
                [0] * 4 + [D] * R,                            # 5: closed by the read's end, L - start == min_run
                [0] * 4 + [D] * (R - 1),                      # 6: ... == min_run - 1
                [D] * R + [D - 1] + [D] * R,                  # 7: two long runs around one base of min_depth - 1
                [D] * R + [D - 1] + [D] * (R - 1),            # 8: one long, one short
                [D + 2] * R + [0] + [D] * R + [1] + [D] * R]  # 9: three
    flags = {1: 1, 2: 0, 3: 0, 4: 1, 5: 0, 6: 1, 7: 2, 8: 0, 9: 2}
    runs = {1: 1, 2: 1, 3: 1, 4: 0, 5: 1, 6: 1, 7: 2, 8: 2, 9: 3}
    return (_profiles("runs_and_depths_at_the_thresholds", profiles, both_modes(min_depth=D, min_run=R, trim_len=5), flags=flags, runs=runs),)


# ---- lists for the prune ------------------------------------------------------------------------------------------------------------------

PRUNE_CFG = dict(mode=0, margin=5, min_depth=5, min_run=60, trim_len=100)


@functools.lru_cache(maxsize=None)
def prune_list():
    """A list with the string graph's fields drawn by string_graph_util.random_overlaps and intervals inside the reads: under PRUNE_CFG some
    reads are unsupported, some split, some neither, and pruning the split ones leaves further reads unsupported (the chain)."""
    rng = np.random.default_rng(65)
    M = 150
    lens = rng.integers(300, 700, M).astype(np.int64)
    rows, cols, vals = sgu.random_overlaps(rng, M, density=0.12, suffix_range=400)
    vals = vals.astype(OVERLAP_DTYPE)
    for f0, f1, who in (("begQ", "endQ", rows), ("begT", "endT", cols)):
        L = lens[who]
        a = rng.integers(0, L // 2); b = a + rng.integers(20, L // 2)
        vals[f0], vals[f1] = a, np.minimum(b, L)
    return Case("prune_list", lens, rows, cols, vals, [PRUNE_CFG])


def prune_chain(case):
    """pileup -> prune(2) -> pileup -> prune(1) -> pileup on the restatement: [(rows, cols, vals, pileup result)] of the three lists."""
    steps = []
    r, c, v = case.rows, case.cols, case.vals
    for mask in (2, 1, None):
        res = _pileup(case.lens, r, c, v, **case.cfgs[0])
        steps.append((r, c, v, res))
        if mask is not None:
            r, c, v = pu.prune(r, c, v, res[0]["flags"], mask)
    return steps


@functools.lru_cache(maxsize=None)
def all_unsupported_case():
    """Depth below min_depth 50 everywhere: every read is flagged unsupported, prune(1) keeps nothing."""
    lens, rows, cols, vals = _random_list(66, 30, 80)
    return Case("every_read_unsupported", lens, rows, cols, vals, [dict(min_depth=50, min_run=10)], flags={v: 1 for v in range(30)})


def hand_cases():
    return block_edge_cases() + emission_cases() + trim_cases()[:-1] + flag_cases()


def all_cases():
    return wide_key_cases() + degenerate_cases() + block_edge_cases() + emission_cases() + trim_cases() + flag_cases() + (prune_list(), all_unsupported_case())
