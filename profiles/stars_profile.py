"""Resolving stars (elba_resolve_stars, stars.hip) on the layout graph of the string graph's scale tests: string_graph_util.layout_overlaps
(seed 2, 300 000 reads, coverage 8) with 3000 stray reads planted, each overlapping one read the prunes keep and one more new read behind
it, loaded as an edge list.  The pairs of R the rule asks for are the layout's own: the reduction removes them from S as transitive.  The
reduction is run again before every call (the call changes S); times are the calls' own device events, medians of --reps calls after one
warm-up call of each kind.  elba_cut_bridges(1, 3) and elba_cut_weak_overlaps(0.7) are measured in the same process on the same S, for
scale: both run the same scan and scatter.
Usage: python profiles/stars_profile.py OUT.json [--reads N] [--stars N] [--reps N]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))             # the graph generators are the tests' own

import numpy as np  # noqa: E402

import elba_amd  # noqa: E402
import string_graph_util as sg  # noqa: E402


def _median(x):
    x = sorted(x)
    return round(x[len(x) // 2], 4), round(x[0], 4), round(x[-1], 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out")
    ap.add_argument("--reads", type=int, default=300000)
    ap.add_argument("--stars", type=int, default=3000)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    rng = np.random.default_rng(2)
    rows, cols, vals = sg.layout_overlaps(rng, a.reads, 8)
    deg, flags = sg.kept_degrees(a.reads, rows, cols, vals, 0.65)
    ok = np.flatnonzero((flags == 0) & (deg > 0))
    u = np.sort(rng.choice(ok, a.stars, replace=False))
    # a stray read w = M + 2 i overlaps u and the new read w + 1 and nothing else: no walk of two entries makes its pairs transitive
    w = a.reads + 2 * np.arange(a.stars, dtype=np.int64)
    xr = np.concatenate([u, w]); xc = np.concatenate([w, w + 1])
    xv = np.zeros(2 * a.stars, dtype=vals.dtype)
    xv["passed"] = 1
    xv["direction"] = rng.integers(0, 4, 2 * a.stars); xv["directionT"] = rng.integers(0, 4, 2 * a.stars)
    xv["suffix"] = rng.integers(3000, 6000, 2 * a.stars); xv["suffixT"] = rng.integers(3000, 6000, 2 * a.stars)
    rows = np.concatenate([rows, xr]); cols = np.concatenate([cols, xc]); vals = np.concatenate([vals, xv])
    order = np.lexsort((cols, rows))
    rows, cols, vals = rows[order], cols[order], vals[order]
    M = a.reads + 2 * a.stars
    e = elba_amd.Engine(17, 2, 8)
    e.set_overlaps(M, rows, cols, vals)
    res = {"reads": int(M), "pairs": int(len(rows)), "planted": a.stars, "reps": a.reps}
    star_keys = ("centres", "pairs0", "pairs1", "pairs2", "pairs3", "reads_removed", "entries_removed", "rounds_run")
    calls = (("resolve_stars_1", lambda: e.resolve_stars(1), star_keys),
             ("resolve_stars_64", lambda: e.resolve_stars(64), star_keys),
             ("cut_bridges_1_3", lambda: e.cut_bridges(1, 3), ("anchors", "chains", "long_flanks", "bridges", "reads_removed", "entries_removed")),
             ("cut_weak_overlaps_0.7", lambda: e.cut_weak_overlaps(0.7), ("branch_sides", "weak_entries", "entries_removed")))
    tr = []
    for name, call, keys in calls:
        got = []
        for _ in range(a.reps + 1):
            t = e.transitive_reduction(0.65, 1000)
            tr.append(t["ms_total"])
            res["edges_kept"] = int(t["edges_kept"])
            got.append(call())
        st = got[-1]
        res[name] = {"ms_total_median_min_max": _median([c["ms_total"] for c in got[1:]]), "ms_compact_median_min_max": _median([c["ms_compact"] for c in got[1:]]),
                     "counts": dict(nnz_before=int(st["nnz_before"]), nnz_after=int(st["nnz_after"]), **{k: int(st[k]) for k in keys})}
    res["transitive_reduction_ms_total_median_min_max"] = _median(tr[1:])
    e.close()
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
