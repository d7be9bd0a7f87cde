"""The assembly-graph export (elba_export_assembly_links, graph_links.hip) on synthetic string graphs loaded as edge lists, and on the
contig profile's accurate-reads workload.  The call is timed by its own device events (ms_total: table, count pass, scan, the host's look at
the total, emit pass and the copy of the records to the host), medians of --reps calls after one warm-up call.
  branches N   N reads of 32 bases under shuffled ids: paths of 16 reads, and one more read per four paths that overlaps an end read of
               each of them (a branch of degree 4): short columns only, one lane per column
  hubs H D     H reads with D lone neighbours each, beside 2^18 reads in paths: columns of D entries, one wavefront per column
Usage: python profiles/graph_links_profile.py OUT.json [--reps N] [--branches N] [--hubs H D] [--workload]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

import elba_amd  # noqa: E402
from elba_amd.capi import OVERLAP_DTYPE  # noqa: E402

KEYS = ("segments", "candidates", "links", "closures", "twisted", "unplaced", "clamped", "asymmetric")


def _paths(ids, P):
    keep = (np.arange(len(ids) - 1) % P) != P - 1
    return ids[:-1][keep], ids[1:][keep]


def _load(n, x, y):
    rng = np.random.default_rng(3)
    r, c = np.minimum(x, y), np.maximum(x, y)
    o = np.lexsort((c, r))
    v = np.zeros(len(r), dtype=OVERLAP_DTYPE)
    v["passed"] = 1; v["direction"] = 1; v["directionT"] = 2; v["suffix"] = 8; v["suffixT"] = 8
    e = elba_amd.Engine(17, 2, 8)
    e.set_reads(rng.integers(0, 256, 8 * n + 16).astype(np.uint8), np.arange(n, dtype=np.uint64) * 8, np.full(n, 32, dtype=np.uint32))
    e.set_overlaps(n, r[o], c[o], v)
    sg = e.transitive_reduction(0.0, 0)
    assert sg["nnz"] == 2 * len(r)
    return e, sg


def _time(e, reps):
    cs = e.generate_contigs(circular=True, singletons=True)
    e.assembly_links()
    runs = [e.assembly_links()[1] for _ in range(reps)]
    ms = sorted(r["ms_total"] for r in runs)
    return {"contigs": {k: int(cs[k]) for k in ("nreads", "branches", "contigs", "contig_reads")}, "contig_ms_total": round(cs["ms_total"], 4),
            "links_ms_total_median_min_max": [round(ms[len(ms) // 2], 4), round(ms[0], 4), round(ms[-1], 4)], "counts": {k: int(runs[-1][k]) for k in KEYS}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--branches", type=int, default=0)
    ap.add_argument("--hubs", type=int, nargs=2, default=None)
    ap.add_argument("--workload", action="store_true")
    a = ap.parse_args()
    res = []
    rng = np.random.default_rng(1)
    if a.branches:
        n, P = a.branches, 16
        npaths = (n * 64 // 65) // P
        ids = rng.permutation(n).astype(np.int64)
        x, y = _paths(ids[:npaths * P], P)
        nb = min(npaths // 4, n - npaths * P)
        hub = np.repeat(ids[npaths * P:npaths * P + nb], 4)
        x, y = np.concatenate([x, hub]), np.concatenate([y, ids[:4 * nb * P:P]])
        e, sg = _load(n, x, y)
        res.append(dict(graph="branches", reads=n, string_nnz=int(sg["nnz"]), **_time(e, a.reps)))
        e.close()
    if a.hubs:
        H, D = a.hubs
        base = 1 << 18
        n = base + H * (D + 1)
        ids = rng.permutation(n).astype(np.int64)
        x, y = _paths(ids[:base], 16)
        hub = np.repeat(ids[base:base + H], D)
        x, y = np.concatenate([x, hub]), np.concatenate([y, ids[base + H:]])
        e, sg = _load(n, x, y)
        res.append(dict(graph="hubs", hubs=H, degree=D, reads=n, string_nnz=int(sg["nnz"]), **_time(e, a.reps)))
        e.close()
    if a.workload:
        packed, off, lens, _ = elba_amd.synth_reads(1, 4_640_000, 30.0, 8000.0, 2000.0, error_rate=0.005, min_len=1000)
        e = elba_amd.Engine(17, 2, 8)
        e.set_reads(packed, off, lens)
        e.count_kmers(); e.create_kmer_matrix(); e.create_seed_matrix()
        e.align_seeds()
        sg = e.transitive_reduction(0.65, 1000)
        res.append(dict(graph="accurate-17k", reads=int(len(lens)), string_nnz=int(sg["nnz"]), **_time(e, a.reps)))
        e.close()
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
