"""Bubble popping (elba_pop_bubbles, bubbles.hip) on the layout graph of the string graph's scale tests: string_graph_util.layout_overlaps (seed 2,
300 000 reads, coverage 8) with 3000 bubbles planted — two chains of new reads, of different lengths from 1 to 3, between two reads the prunes
keep, 40 reads apart — loaded as an edge list.  The reduction is run again before every call (the calls change S); times are the calls' own
device events, the first call of each kind left out.  elba_clip_tips(3, 2) runs on the same graph in the same process as the yardstick: its
ms_compact is the same compaction of the same S.  --hub N adds one pair of anchors joined by N one-read arms, the quadratic case of the pick
(run that one under a kernel trace to see k_bub_pick alone; here it shows in ms_total less ms_compact).
Usage: python profiles/bubbles_profile.py OUT.json [--reads N] [--bubbles N] [--reps N] [--hub N]"""
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
import tip_util as tu  # noqa: E402


def _median(x):
    x = sorted(x)
    return round(x[len(x) // 2], 4), round(x[0], 4), round(x[-1], 4)


def _calls(e, reps, cutoff, fuzz, call, keys):
    out, tr = [], []
    for _ in range(reps + 1):
        tr.append(e.transitive_reduction(cutoff, fuzz)["ms_total"])
        out.append(call())
    st = out[-1]
    return {"ms_total_median_min_max": _median([c["ms_total"] for c in out[1:]]), "ms_compact_median_min_max": _median([c["ms_compact"] for c in out[1:]]),
            "counts": {k: int(st[k]) for k in keys}}, tr[1:]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out")
    ap.add_argument("--reads", type=int, default=300000)
    ap.add_argument("--bubbles", type=int, default=3000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--hub", type=int, default=3000)
    a = ap.parse_args()
    bkeys = ("nnz_before", "nnz_after", "anchors", "arms", "bubbles", "arms_removed", "reads_removed", "entries_removed", "rounds_run")
    res = {"reps": a.reps, "calls": []}
    e = elba_amd.Engine(17, 2, 8)
    if a.reads:
        rng = np.random.default_rng(2)
        rows, cols, vals = sg.layout_overlaps(rng, a.reads, 8)
        deg, flags = sg.kept_degrees(a.reads, rows, cols, vals, 0.65)
        ok = np.flatnonzero((flags[:-40] == 0) & (deg[:-40] > 0) & (flags[40:] == 0) & (deg[40:] > 0))
        u = np.sort(rng.choice(ok, a.bubbles, replace=False))
        lengths = np.array([[1, 2], [1, 3], [2, 3]])[rng.integers(0, 3, a.bubbles)].reshape(-1)
        M, rows, cols, vals, _ = bu.plant_bubbles(rng, a.reads, rows, cols, vals, [(int(x), int(x) + 40) for x in u for _ in range(2)], lengths)
        e.set_overlaps(M, rows, cols, vals)
        res.update(reads=int(M), pairs=int(len(rows)))
        tr = []
        for rounds in (2, 64):
            r, t = _calls(e, a.reps, 0.65, 1000, lambda: e.pop_bubbles(3, rounds), bkeys)
            r.update(call="pop_bubbles", max_arm_reads=3, rounds=rounds)
            res["calls"].append(r); tr += t
        r, t = _calls(e, a.reps, 0.65, 1000, lambda: e.clip_tips(3, 2), ("nnz_before", "nnz_after", "dead_ends", "tips", "reads_removed", "entries_removed", "rounds_run"))
        r.update(call="clip_tips", max_tip_reads=3, rounds=2)
        res["calls"].append(r); tr += t
        res["transitive_reduction_ms_total_median_min_max"] = _median(tr)
    if a.hub:
        g = tu.Graph()
        bu._bubble(g, [1] * a.hub)
        M, rows, cols, vals = g.overlaps(np.random.default_rng(a.hub))
        e.set_overlaps(M, rows, cols, vals)
        r, _ = _calls(e, a.reps, 0.0, 0, lambda: e.pop_bubbles(1, 1), bkeys)
        r.update(call="pop_bubbles", graph="one pair of anchors, %d one-read arms" % a.hub, max_arm_reads=1, rounds=1)
        res["calls"].append(r)
    e.close()
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
