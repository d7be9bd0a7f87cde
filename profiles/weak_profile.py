"""Cutting weak overlaps (elba_cut_weak_overlaps, weak.hip) on the layout graph of the string graph's scale tests: string_graph_util.layout_overlaps
(seed 2, 300 000 reads, coverage 8) with 3000 overlaps of score 1 planted between reads the prunes keep, 1000 reads apart, loaded as an edge
list.  The reduction is run again before every call (the call changes S); times are the calls' own device events, the first call of each
kind left out.  elba_clip_tips(3, 1) is measured in the same process on the same S: its compaction is the same scatter over the same bytes.
Usage: python profiles/weak_profile.py OUT.json [--reads N] [--weak N] [--reps N] [--ratio R]"""
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
import weak_util as wu  # noqa: E402


def _median(x):
    x = sorted(x)
    return round(x[len(x) // 2], 4), round(x[0], 4), round(x[-1], 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out")
    ap.add_argument("--reads", type=int, default=300000)
    ap.add_argument("--weak", type=int, default=3000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--ratio", type=float, default=0.7)
    a = ap.parse_args()
    rng = np.random.default_rng(2)
    rows, cols, vals = sg.layout_overlaps(rng, a.reads, 8)
    deg, flags = sg.kept_degrees(a.reads, rows, cols, vals, 0.65)
    ok = np.flatnonzero((flags[:-1000] == 0) & (deg[:-1000] > 0) & (flags[1000:] == 0) & (deg[1000:] > 0))
    u = np.sort(rng.choice(ok, a.weak, replace=False))
    rows, cols, vals = wu.plant_weak_edges(a.reads, rows, cols, vals, [(int(x), int(x) + 1000) for x in u], 1, rng.integers(0, 4, (a.weak, 2)).tolist())
    M = a.reads
    e = elba_amd.Engine(17, 2, 8)
    e.set_overlaps(M, rows, cols, vals)
    res = {"reads": int(M), "pairs": int(len(rows)), "planted": a.weak, "reps": a.reps, "min_ratio_q16": wu.q16_of(a.ratio)}
    tr, cuts, clips = [], [], []
    for _ in range(a.reps + 1):
        tr.append(e.transitive_reduction(0.65, 1000)["ms_total"])
        cuts.append(e.cut_weak_overlaps(a.ratio))
    for _ in range(a.reps + 1):
        tr.append(e.transitive_reduction(0.65, 1000)["ms_total"])
        clips.append(e.clip_tips(3, 1))
    st = cuts[-1]
    mc = _median([c["ms_compact"] for c in cuts[1:]])
    moved = (st["nnz_before"] + st["nnz_after"]) * 52        # the scatter reads nnz entries of 52 bytes and writes the kept ones
    res["cut_weak_overlaps"] = {"ms_total_median_min_max": _median([c["ms_total"] for c in cuts[1:]]), "ms_compact_median_min_max": mc,
                                "compact_gb_per_s_at_median": round(moved / (mc[0] * 1e-3) / 1e9, 1) if mc[0] > 0 else None,
                                "counts": {k: int(st[k]) for k in wu.STATS}}
    tp = clips[-1]
    res["clip_tips_3_1"] = {"ms_total_median_min_max": _median([c["ms_total"] for c in clips[1:]]), "ms_compact_median_min_max": _median([c["ms_compact"] for c in clips[1:]]),
                            "counts": {k: int(tp[k]) for k in ("nnz_before", "nnz_after", "tips", "reads_removed", "entries_removed")}}
    res["transitive_reduction_ms_total_median_min_max"] = _median(tr[1:])
    e.close()
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
