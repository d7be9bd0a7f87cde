"""Component stage (elba_graph_components, components.hip) on both graphs of one layout-shaped overlap graph: reads placed on a genome
(tests/string_graph_util.layout_overlaps, 200 000 reads at coverage 8 by default), loaded as an edge list, reduced to S.  The stage is
timed by its own device events (ms_total, ms_label) on calls after a warm-up call, and its passes are recorded; beside them the wall time
of the vectorised host form of the same rule (tests/comp_util.min_label) on the same edges, and of elba_partition_components.
Usage: python profiles/components_profile.py OUT.json [--reads N] [--coverage C] [--reps N]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402

import comp_util as ku  # noqa: E402
import elba_amd  # noqa: E402
import string_graph_util as sg  # noqa: E402


def _median(xs):
    xs = sorted(xs)
    return round(xs[len(xs) // 2], 4)


def run(M, cov, reps):
    t0 = time.time()
    rows, cols, vals = sg.layout_overlaps(np.random.default_rng(1), M, cov)
    e = elba_amd.Engine(17, 2, 8)
    e.set_overlaps(M, rows, cols, vals)
    st = e.transitive_reduction(0.65, 1000)
    g = e.export_string_graph()
    edges = {"string": ku.edges_of_string_graph(g), "overlaps": ku.edges_of_overlaps(rows, cols, vals)}
    out = {"reads": int(M), "coverage": cov, "pairs": int(len(rows)), "string_nnz": int(st["nnz"]), "reps": reps, "graphs": {}}
    for graph in ("string", "overlaps"):
        e.graph_components(graph)                            # warm-up: buffers allocated
        runs = [e.graph_components(graph)[1] for _ in range(reps)]
        t1 = time.time()
        labels, rounds = ku.min_label(M, *edges[graph])
        host_s = time.time() - t1
        t1 = time.time()
        part, pw = e.partition_components(8, graph=graph, nreads=M)
        part_s = time.time() - t1
        last = runs[-1]
        assert last["components"] == int((labels == np.arange(M)).sum())
        nnz = int(st["nnz"]) if graph == "string" else int(len(rows))
        out["graphs"][graph] = {
            "edges": int(last["edges"]), "components": int(last["components"]), "used_components": int(last["used_components"]), "largest_reads": int(last["largest_reads"]),
            "passes": int(last["passes"]), "ms_total_median": _median(r["ms_total"] for r in runs), "ms_total_min": round(min(r["ms_total"] for r in runs), 4),
            "ms_label_median": _median(r["ms_label"] for r in runs), "ms_label_min": round(min(r["ms_label"] for r in runs), 4),
            # algorithmic bytes of one call (components.hip's header): three passes over the entries at 16 (+ 1) bytes, the column pointers of S at 8,
            # the passes over the reads, the tables cleared and copied out
            "algorithmic_bytes": int(nnz * (3 * 16 + (8 if graph == "string" else 3)) + M * (8 * (3 + 1) + 8 + 16 + 48) + 56 * last["components"]),
            "host_min_label_s": round(host_s, 4), "host_min_label_rounds": int(rounds), "partition_8_parts_wall_s": round(part_s, 4),
            "part_weight": [int(x) for x in pw]}
    e.close()
    out["wall_s"] = round(time.time() - t0, 1)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out")
    ap.add_argument("--reads", type=int, default=200000)
    ap.add_argument("--coverage", type=int, default=8)
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    res = run(a.reads, a.coverage, a.reps)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
