"""Tip clipping (elba_clip_tips, tips.hip) on the layout graph of the string graph's scale tests: string_graph_util.layout_overlaps (seed 2,
300 000 reads, coverage 8) with 3000 tips of 1 to 3 new reads planted at reads the prunes keep, loaded as an edge list.  The reduction is
run again before every clip (the call changes S); times are the calls' own device events, the first call of each kind left out.
Usage: python profiles/tips_profile.py OUT.json [--reads N] [--tips N] [--reps N]"""
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
import tip_util as tu  # noqa: E402


def _median(x):
    x = sorted(x)
    return round(x[len(x) // 2], 4), round(x[0], 4), round(x[-1], 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out")
    ap.add_argument("--reads", type=int, default=300000)
    ap.add_argument("--tips", type=int, default=3000)
    ap.add_argument("--reps", type=int, default=7)
    a = ap.parse_args()
    rng = np.random.default_rng(2)
    rows, cols, vals = sg.layout_overlaps(rng, a.reads, 8)
    deg, flags = sg.kept_degrees(a.reads, rows, cols, vals, 0.65)
    anchors = np.sort(rng.choice(np.flatnonzero((flags == 0) & (deg > 0)), a.tips, replace=False))
    M, rows, cols, vals, _ = tu.plant_tips(rng, a.reads, rows, cols, vals, anchors, rng.integers(1, 4, a.tips))
    e = elba_amd.Engine(17, 2, 8)
    e.set_overlaps(M, rows, cols, vals)
    res = {"reads": int(M), "pairs": int(len(rows)), "reps": a.reps, "calls": []}
    tr = []
    for rounds in (2, 64):
        clips = []
        for _ in range(a.reps + 1):
            tr.append(e.transitive_reduction(0.65, 1000)["ms_total"])
            clips.append(e.clip_tips(3, rounds))
        st = clips[-1]
        moved = (st["nnz_before"] + st["nnz_after"]) * 52      # the first round's compaction reads nnz entries of 52 bytes and writes the kept ones (2 rounds: all of them)
        mt, mc = _median([c["ms_total"] for c in clips[1:]]), _median([c["ms_compact"] for c in clips[1:]])
        res["calls"].append({"max_tip_reads": 3, "rounds": rounds, "ms_total_median_min_max": mt, "ms_compact_median_min_max": mc,
                             "compact_gb_per_s_at_median": round(moved / (mc[0] * 1e-3) / 1e9, 1) if rounds == 2 and mc[0] > 0 else None,
                             "counts": {k: int(st[k]) for k in ("nnz_before", "nnz_after", "dead_ends", "tips", "reads_removed", "entries_removed", "spared_anchors", "rounds_run")}})
    res["transitive_reduction_ms_total_median_min_max"] = _median(tr[1:])
    e.close()
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
