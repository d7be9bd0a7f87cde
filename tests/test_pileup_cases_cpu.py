"""CPU: every case of pileup_cases.py holds what it claims, computed from the pair list and the restatement (pileup_util.py) alone, and the
vectorised restatement equals the literal loops at the sizes the GPU tests lean on it: GetTrimmedInterval base by base, and the per-base
depth counted interval by interval.  A case that misses its claim fails here, before test_gpu_pileup_edges.py spends GPU time on it."""
import numpy as np
import pytest

import pileup_cases as pc
import pileup_util as pu

BRUTE_MAX = 2**20


def _ids(cases):
    return [c.name for c in cases]


def _endpoints(case, cfg):
    """(reads, positions) of the credited endpoints, starts then ends."""
    reads, beg, end, used = pu.intervals(*case.args, mode=cfg["mode"], margin=cfg["margin"])
    return np.concatenate([reads, reads]), np.concatenate([beg, end])


def _segs(p, v):
    a, b = int(p["seg_off"][v]), int(p["seg_off"][v + 1])
    return [(int(s), int(d)) for s, d in zip(p["seg_start"][a:b], p["seg_depth"][a:b])]


def _brute_depth(case, cfg, v):
    """Depth of read v by a plain loop over the accepted pairs' intervals."""
    d = np.zeros(int(case.lens[v]), np.int64)
    acc = pu.accepted(case.vals, cfg["mode"])
    m = cfg["margin"]
    for who, fb, fe in ((case.rows, "begQ", "endQ"), (case.cols, "begT", "endT")):
        for a in np.flatnonzero(acc & (who == v)):
            b, e = int(case.vals[fb][a]) + m, int(case.vals[fe][a]) - m
            if b < e:
                d[b:e] += 1
    return d


@pytest.mark.parametrize("case", pc.all_cases(), ids=_ids(pc.all_cases()))
def test_pair_list_is_loadable(case):
    """elba_set_overlaps' rule: 0 <= row < col < M, strictly ascending in (row, col); intervals inside [0, len] with beg <= end."""
    M = len(case.lens)
    r, c, v = case.rows, case.cols, case.vals
    assert len(r) == len(c) == len(v)
    assert ((0 <= r) & (r < c) & (c < M)).all()
    key = r * (M + 1) + c
    assert (np.diff(key) > 0).all()
    for who, fb, fe in ((r, "begQ", "endQ"), (c, "begT", "endT")):
        assert ((0 <= v[fb]) & (v[fb] <= v[fe]) & (v[fe] <= case.lens[who])).all()
    assert 4 * len(r) + M < 2**31


@pytest.mark.parametrize("case", pc.all_cases(), ids=_ids(pc.all_cases()))
def test_case_holds_its_claims(case):
    cfg = case.cfgs[0]
    cl = case.claims
    p, st, depth, off = pc.reference(case, cfg)
    er, ep = _endpoints(case, cfg)
    if "E" in cl:
        assert len(er) == cl["E"] and st["intervals"] * 2 == cl["E"]
    if "key_bits" in cl:
        mb, pb = pc.key_bits(case.lens)
        assert mb + pb + 1 == cl["key_bits"]
        assert -(-cl["key_bits"] // 8) == (4 if cl["key_bits"] <= 32 else 5)          # the sort's passes of 8-bit digits
        assert ((er >> (mb - 1)) & 1).any() and ((ep >> (pb - 1)) & 1).any()
        keys = (er << (pb + 1)) | (ep << 1)
        assert int(keys.max()).bit_length() == cl["key_bits"]
        assert (ep == case.lens[er]).any()                                             # an interval ends exactly at len
        for c2 in case.cfgs:                                                            # both settings differ in what they accept
            assert pc.reference(case, c2)[1]["intervals"] > 400
    for k, want in cl.get("stats", {}).items():
        for c2 in case.cfgs[:2]:
            assert pc.reference(case, c2)[1][k] == want, (k, c2)
    if "longest" in cl:
        assert pc.reference(case, case.cfgs[2])[1]["intervals"] > 0                    # one less margin and an interval survives
    if "max_depth" in cl:
        assert st["max_depth"] == cl["max_depth"]
    for v, want in cl.get("segs", {}).items():
        assert _segs(p, v) == want, v
    for v, want in cl.get("profile", {}).items():
        assert depth[off[v]:off[v + 1]].tolist() == want, v
    for v, want in cl.get("trim", {}).items():
        assert (int(p["trim_beg"][v]), int(p["trim_end"][v])) == want, v
    for v, want in cl.get("flags", {}).items():
        assert int(p["flags"][v]) == want, v
    for v, want in cl.get("runs", {}).items():
        s, e = pu._runs(depth[off[v]:off[v + 1]], cfg["min_depth"])
        assert len(s) == want, v
    if "curbases" in cl:
        d = depth[off[0]:off[1]]
        s, e = pu._runs(d, cfg["min_depth"])
        assert max(int(d[a:b].sum()) for a, b in zip(s, e)) == cl["curbases"] > 2**31


def test_groups_reach_the_shapes_they_name():
    """The block-edge cases cover E < M, E == M and E > M at every E; the emission cases have no boundary where ends and starts balance."""
    seen = {}
    for c in pc.block_edge_cases():
        E, M = c.claims["E"], len(c.lens)
        seen.setdefault(E, set()).add(M)
    assert sorted(seen) == [2, 254, 256, 258, 510, 512, 514]
    for E, Ms in seen.items():
        assert {E, E + 1} <= Ms and (E == 2 or E - 1 in Ms)
    assert {255, 256, 257} <= seen[2]
    names = {c.name: c for c in pc.emission_cases()}
    for k in (1, 64, 3000):
        bal = names["mid_%d_ends_%d_starts" % (k, k)]
        r = len(bal.lens) // 2
        assert 20 not in [s for s, _ in bal.claims["segs"][r]]
        for j in (k - 1, k + 1):
            c = names["mid_%d_ends_%d_starts" % (k, j)]
            assert (20, j) in c.claims["segs"][len(c.lens) // 2]
    # the trim_len range: every setting's result, by hand (the profile is [0]*3 + [2]*10 + [3]*7 + [0]*2; one run of 17 bases from 3)
    c = {c.name: c for c in pc.trim_cases()}["trim_len_range"]
    got = [tuple(int(pc.reference(c, cfg)[0][k][1]) for k in ("trim_beg", "trim_end")) for cfg in c.cfgs]
    assert got == [(3, 20), (3, 20), (-1, -1), (-1, -1), (-1, -1), (3, 20), (-1, -1)]


@pytest.mark.parametrize("case", pc.all_cases(), ids=_ids(pc.all_cases()))
def test_restatement_equals_the_literal_loops(case):
    """On every read of the hand cases and the long reads of the large ones: trimmed_interval == trimmed_interval_literal(fixed=True), and
    the depth rebuilt from the segments == the interval-by-interval count."""
    for cfg in case.cfgs:
        p, st, depth, off = pc.reference(case, cfg)
        reads = range(len(case.lens)) if case.reads is None else case.reads
        for v in reads:
            d = depth[off[v]:off[v + 1]]
            assert pu.trimmed_interval(d, cfg["min_depth"], cfg["trim_len"]) == pu.trimmed_interval_literal(d.tolist(), cfg["min_depth"], cfg["trim_len"], fixed=True), (v, cfg)
            assert (int(p["trim_beg"][v]), int(p["trim_end"][v])) == pu.trimmed_interval(d, cfg["min_depth"], cfg["trim_len"])
            if case.lens[v] <= BRUTE_MAX:
                rebuilt = pu.profile_of(p["seg_off"], p["seg_start"], p["seg_depth"], case.lens, v)
                assert len(rebuilt) == case.lens[v] and (rebuilt == _brute_depth(case, cfg, v)).all(), (v, cfg)


def test_two_prunes_equal_one_prune_of_the_union():
    case = pc.prune_list()
    (r0, c0, v0, res0), (r1, c1, v1, res1), (r2, c2, v2, res2) = pc.prune_chain(case)
    f0, f1 = res0[0]["flags"], res1[0]["flags"]
    assert set(np.unique(f0).tolist()) == {0, 1, 2}                                     # every kind of read is there
    assert len(r0) > len(r1) > len(r2) > 0                                              # both prunes remove pairs and pairs remain
    union = (((f0 & 2) != 0) | ((f1 & 1) != 0)).astype(np.uint8)
    ru, cu_, vu = pu.prune(r0, c0, v0, union, 1)
    assert (ru == r2).all() and (cu_ == c2).all() and (vu == v2).all()
    assert not (union[r2] | union[c2]).any()
    # the masks the GPU test walks keep different lists
    kept = {m: len(pu.prune(r0, c0, v0, f0, m)[0]) for m in (0, 1, 2, 3, 4, 255)}
    assert kept[0] == kept[4] == len(r0) and kept[3] == kept[255] < min(kept[1], kept[2]) and kept[1] != kept[2]
    # and the case that keeps nothing
    none = pc.all_unsupported_case()
    fl = pc.reference(none, none.cfgs[0])[0]["flags"]
    assert (fl == 1).all() and len(pu.prune(none.rows, none.cols, none.vals, fl, 1)[0]) == 0
