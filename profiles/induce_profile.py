"""Induce stage (elba_induce_part, induce.hip): the 3000-read multi-component input of tests/test_gpu_induce.py and one layout-shaped
overlap graph (tests/string_graph_util.layout_overlaps, 20 000 reads at coverage 8 by default) with reads of `--length` bases, partitioned
by the components of its passed pairs; every part is cut out `--reps` times after a warm-up call and timed by the stage's own device events
(ms_total, ms_pairs, ms_gather).  The gather's rate is its algorithmic bytes (2 x bases / 4 + 16 per read) over ms_gather.
Usage: python profiles/induce_profile.py OUT.json [--reads N] [--coverage C] [--length L] [--parts P] [--reps N]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402

import contig_util as cu  # noqa: E402
import elba_amd  # noqa: E402
import induce_util as iu  # noqa: E402
import string_graph_util as sg  # noqa: E402


def _median(xs):
    xs = sorted(xs)
    return round(xs[len(xs) // 2], 4)


def measure(e, M, npairs, nparts, reps):
    part_of_read, weight = e.partition_components(nparts, graph="overlaps", min_reads=1, nreads=M)
    parts = []
    for p in range(nparts):
        e.induce_part(part_of_read, p, host=False)          # warm-up: buffers allocated
        runs = [e.induce_part(part_of_read, p, host=False)[1] for _ in range(reps)]
        last = runs[-1]
        gather_bytes = 2 * (last["bases"] // 4) + 16 * last["reads"]
        ms_g = _median(r["ms_gather"] for r in runs)
        parts.append({"part": p, "reads": int(last["reads"]), "pairs": int(last["pairs"]), "bases": int(last["bases"]), "packed_bytes": int(last["packed_bytes"]),
                      "split_pairs": int(last["split_pairs"]), "split_passed": int(last["split_passed"]),
                      "ms_total_median": _median(r["ms_total"] for r in runs), "ms_total_min": round(min(r["ms_total"] for r in runs), 4),
                      "ms_pairs_median": _median(r["ms_pairs"] for r in runs), "ms_gather_median": ms_g, "ms_gather_min": round(min(r["ms_gather"] for r in runs), 4),
                      "gather_algorithmic_bytes": int(gather_bytes), "gather_GBps_median": round(gather_bytes / (ms_g * 1e6), 1) if ms_g > 0 else None,
                      "pairs_algorithmic_bytes": int(17 * npairs + 104 * last["pairs"])})
    return {"reads": int(M), "pairs": int(npairs), "nparts": nparts, "reps": reps, "parts": parts}


def run(M, cov, L, nparts, reps):
    t0 = time.time()
    out = {}
    g = iu.build_input(12, (("layout", 900), ("layout", 700), ("layout", 500), ("layout", 400), ("layout", 300), ("layout", 150), ("layout", 40), ("layout", 7)), n_failed=400, lone=5)
    e = elba_amd.Engine(17, 2, 8)
    e.set_reads(*g["reads"])
    e.set_overlaps(g["M"], g["rows"], g["cols"], g["vals"])
    out["built_3000"] = measure(e, g["M"], len(g["rows"]), 3, reps)
    rng = np.random.default_rng(1)
    rows, cols, vals = sg.layout_overlaps(rng, M, cov)
    packed, off, lens = cu.random_packed(rng, M, L, L)
    e.set_reads(packed, off, lens)
    e.set_overlaps(M, rows, cols, vals)
    out["layout"] = dict(measure(e, M, len(rows), nparts, reps), coverage=cov, read_length=L)
    e.close()
    out["wall_s"] = round(time.time() - t0, 1)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out")
    ap.add_argument("--reads", type=int, default=20000)
    ap.add_argument("--coverage", type=int, default=8)
    ap.add_argument("--length", type=int, default=10000)
    ap.add_argument("--parts", type=int, default=2)
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    res = run(a.reads, a.coverage, a.length, a.parts, a.reps)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
