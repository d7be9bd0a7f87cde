"""CPU: the two restatements of the weak-overlap rule (weak_util.py) against each other, the hand cases against what they claim, and the
properties include/elba_amd.h states: the pass is its own fixed point, the removed set grows with the ratio, names do not matter, a
symmetric S stays symmetric, and an entry that ties the best of its side at both its ends is never removed."""
import numpy as np
import pytest

import contig_util as cu
import weak_util as wu

CASES = wu.hand_cases()
RATIOS = (1, 16384, 32768, wu.Q07, 65536)


def _random(seed):
    rng = np.random.default_rng(seed)
    M = int(rng.integers(2, 40))
    (rows, cols, vals), S = wu.random_S(rng, M, p_one_image=0.0 if seed % 3 == 0 else 0.08)
    return M, (rows, cols, vals), S


def _pairs(rows, cols):
    return {(int(r), int(c)) for r, c in zip(rows, cols)}


@pytest.mark.parametrize("name", sorted(CASES))
def test_hand_cases_show_what_they_claim(name):
    case = CASES[name]
    (M, rows, cols, vals), S = wu.case_S(case, np.random.default_rng(1), extra_reads=2)
    assert ((vals["suffix"] >= 5) & (vals["suffix"] <= 9) & (vals["suffixT"] >= 5) & (vals["suffixT"] <= 9)).all()
    trace = {}
    got = wu.cut_weak(M, S[0], S[1], S[2], case["q16"], trace)
    assert wu.same(got, wu.cut_weak_sorted(M, S[0], S[1], S[2], case["q16"]))
    for k, n in case["cnt"].items():
        assert trace["cnt"][k] == n, (k, trace["cnt"][k])
    for k, b in case["best"].items():
        assert trace["best"][k] == b, (k, trace["best"][k])
    assert trace["weak"] == case["weak"]
    assert {frozenset(p) for p in trace["removed"]} == case["removed"]
    st = got[3]
    assert st["weak_entries"] == len(case["weak"]) and st["branch_sides"] == case["branch_sides"] and st["sides_emptied"] == case["sides_emptied"]
    assert st["nnz_after"] == st["nnz_before"] - st["entries_removed"] == len(got[0])
    assert _pairs(S[0], S[1]) - _pairs(got[0], got[1]) == trace["removed"]


def test_hand_cases_cover_the_clauses():
    sizes = {name: len(c["removed"]) for name, c in CASES.items()}
    assert sum(1 for n in sizes.values() if n == 0) >= 6 and sum(1 for n in sizes.values() if n > 0) >= 8
    one = [c for c in CASES.values() if any(a[3] for a in c["graph"].attr.values())]
    assert len(one) == 2
    for c in one:                                               # the pair really has one image
        (M, rows, cols, vals), S = wu.case_S(c, np.random.default_rng(1))
        assert len(S[0]) == 2 * len(rows) - 1
    lo = [s for c in CASES.values() for s, _, _, _ in c["graph"].attr.values()]
    assert min(lo) == -2 ** 31 and max(lo) == 2 ** 31 - 1 and 0 in lo


def test_the_two_restatements_agree_on_300_random_graphs():
    removed = 0
    for seed in range(300):
        M, _, S = _random(seed)
        q16 = RATIOS[seed % len(RATIOS)]
        a = wu.cut_weak(M, S[0], S[1], S[2], q16)
        assert wu.same(a, wu.cut_weak_sorted(M, S[0], S[1], S[2], q16)), seed
        removed += a[3]["entries_removed"]
    assert removed > 300


def test_a_second_pass_with_the_same_ratio_removes_nothing():
    for seed in range(120):
        M, _, S = _random(seed)
        for q16 in RATIOS:
            a = wu.cut_weak(M, S[0], S[1], S[2], q16)
            b = wu.cut_weak(M, a[0], a[1], a[2], q16)
            assert b[3]["entries_removed"] == 0 and b[3]["weak_entries"] == 0 and wu.same((b[0], b[1], b[2], None), (a[0], a[1], a[2], None)), (seed, q16)


def test_the_removed_set_grows_with_the_ratio():
    strict = 0
    for seed in range(120):
        M, _, S = _random(seed)
        kept = [_pairs(*wu.cut_weak(M, S[0], S[1], S[2], q16)[:2]) for q16 in sorted(RATIOS)]
        for small, large in zip(kept[:-1], kept[1:]):
            assert large <= small, seed
            strict += large < small
    assert strict > 100


def test_the_removed_pairs_do_not_depend_on_the_names_of_the_reads():
    for seed in range(100):
        rng = np.random.default_rng(1000 + seed)
        M, (rows, cols, vals), S = _random(seed)
        perm = rng.permutation(M)
        S2 = wu.S_of(*wu.relabel_upper(perm, rows, cols, vals))
        assert len(S2[0]) == len(S[0])
        for q16 in (wu.Q07, 65536):
            a = wu.cut_weak(M, S[0], S[1], S[2], q16)
            b = wu.cut_weak(M, S2[0], S2[1], S2[2], q16)
            assert {(int(perm[r]), int(perm[c])) for r, c in _pairs(a[0], a[1])} == _pairs(b[0], b[1]), seed
            assert all(a[3][k] == b[3][k] for k in wu.STATS)


def test_a_symmetric_S_stays_symmetric():
    for seed in range(0, 120, 3):                               # the seeds without one-image pairs
        M, _, S = _random(seed)
        assert _pairs(S[0], S[1]) == _pairs(S[1], S[0])
        for q16 in (wu.Q07, 65536):
            r, c, v, st = wu.cut_weak(M, S[0], S[1], S[2], q16)
            ent = {(int(a), int(b)): o for a, b, o in zip(r, c, v)}
            assert st["entries_removed"] % 2 == 0
            for (a, b), o in ent.items():
                assert cu.transpose(o).tobytes() == ent[(b, a)].tobytes()


def test_an_entry_that_ties_the_best_at_both_its_ends_is_never_removed():
    seen = 0
    for seed in range(150):
        M, _, S = _random(seed)
        rows, cols, vals = S
        side = vals["direction"] & 1
        best = {}
        for r, c, e, s in zip(rows, cols, side, vals["score"]):
            best[(int(c), int(e))] = max(best.get((int(c), int(e)), -2 ** 40), int(s))
        at = {(int(r), int(c)): z for z, (r, c) in enumerate(zip(rows, cols))}
        safe = set()
        for (r, c), z in at.items():
            m = at.get((c, r))
            if int(vals["score"][z]) == best[(c, int(side[z]))] and (m is None or int(vals["score"][m]) == best[(r, int(side[m]))]):
                safe.add((r, c))
        for q16 in (1, wu.Q07, 65536):
            got = wu.cut_weak(M, rows, cols, vals, q16)
            assert safe <= _pairs(got[0], got[1]), (seed, q16)
        seen += len(safe)
    assert seen > 500


def test_the_binding_has_the_call_and_refuses_a_bad_ratio_before_the_library():
    import ctypes as C

    import elba_amd
    from elba_amd import capi
    assert C.sizeof(capi.WeakCfg) == 16 and C.sizeof(capi.WeakStats) == 7 * 8 + 2 * 4
    assert [f[0] for f in capi.WeakStats._fields_][:7] == list(wu.STATS)
    e = object.__new__(elba_amd.Engine)                         # no context, no library: a bad ratio must not get that far
    for bad in (0.0, -0.5, 1.00001, 0.000007, 2):
        with pytest.raises(ValueError):
            e.cut_weak_overlaps(bad)
    assert wu.q16_of(0.7) == wu.Q07 and wu.q16_of(1.0) == 65536 and wu.q16_of(0.00001) == 1
