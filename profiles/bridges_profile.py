"""Cutting bridges (elba_cut_bridges, bridges.hip) on the layout graph of the string graph's scale tests: string_graph_util.layout_overlaps
(seed 2, 300 000 reads, coverage 8) with 3000 one-read chains planted between reads the prunes keep, 1000 reads apart, loaded as an edge
list.  The reduction is run again before every call (the call changes S); times are the calls' own device events, medians of --reps calls
after one warm-up call of each kind.  elba_pop_bubbles(3, 1) and elba_cut_weak_overlaps(0.7) are measured in the same process on the same
S, for scale: the first walks the same chains, both run the same scan and scatter.
Usage: python profiles/bridges_profile.py OUT.json [--reads N] [--bridges N] [--reps N]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))             # the graph generators are the tests' own

import numpy as np  # noqa: E402

import bubble_util as bu  # noqa: E402
import elba_amd  # noqa: E402
import string_graph_util as sg  # noqa: E402


def _median(x):
    x = sorted(x)
    return round(x[len(x) // 2], 4), round(x[0], 4), round(x[-1], 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out")
    ap.add_argument("--reads", type=int, default=300000)
    ap.add_argument("--bridges", type=int, default=3000)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    rng = np.random.default_rng(2)
    rows, cols, vals = sg.layout_overlaps(rng, a.reads, 8)
    deg, flags = sg.kept_degrees(a.reads, rows, cols, vals, 0.65)
    ok = np.flatnonzero((flags[:-1000] == 0) & (deg[:-1000] > 0) & (flags[1000:] == 0) & (deg[1000:] > 0))
    u = np.sort(rng.choice(ok, a.bridges, replace=False))
    # (a planted read has two neighbours 1000 reads apart that share no pair, so no walk of two entries makes its pairs transitive)
    M, rows, cols, vals, planted = bu.plant_bubbles(rng, a.reads, rows, cols, vals, [(int(x), int(x) + 1000) for x in u], [1] * a.bridges)
    e = elba_amd.Engine(17, 2, 8)
    e.set_overlaps(M, rows, cols, vals)
    res = {"reads": int(M), "pairs": int(len(rows)), "planted": a.bridges, "reps": a.reps}
    calls = (("cut_bridges_1_3", lambda: e.cut_bridges(1, 3), ("anchors", "chains", "long_flanks", "bridges", "reads_removed", "entries_removed")),
             ("cut_bridges_3_50", lambda: e.cut_bridges(3, 50), ("anchors", "chains", "long_flanks", "bridges", "reads_removed", "entries_removed")),
             ("pop_bubbles_3_1", lambda: e.pop_bubbles(3, 1), ("anchors", "arms", "bubbles", "reads_removed", "entries_removed")),
             ("cut_weak_overlaps_0.7", lambda: e.cut_weak_overlaps(0.7), ("branch_sides", "weak_entries", "entries_removed")))
    tr = []
    for name, call, keys in calls:
        got = []
        for _ in range(a.reps + 1):
            tr.append(e.transitive_reduction(0.65, 1000)["ms_total"])
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
