"""Contig stage (elba_generate_contigs, contig.hip) on two workloads: reads -> B -> x-drop alignments -> string graph -> contigs on one GPU.
The stage is timed by its own device events (ms_total, ms_rank) on calls after a warm-up call; the string graph's stage time is recorded beside
it.  Usage: python profiles/contig_profile.py OUT.json [--reps N]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

import elba_amd  # noqa: E402

WORKLOADS = {
    # accurate reads on an E. coli-sized genome: 17 400 reads like the string-graph line of DESIGN §4.6 (19 825 aligned pairs here, not its 548 373)
    "accurate-17k": dict(genome=4_640_000, depth=30.0, avg_len=8000.0, sd_len=2000.0, min_len=1000, error=0.005, k=17, lower=2, upper=8, seed=1),
    # BASELINE.json configs[1] (16 893 reads; bench.py --workload ecsample30x-like)
    "ecsample30x-like": dict(genome=4_640_000, depth=30.0, avg_len=8240.0, sd_len=2000.0, min_len=1000, error=0.15, k=17, lower=2, upper=8, seed=1),
}


def run(name, w, reps):
    t0 = time.time()
    packed, off, lens, _ = elba_amd.synth_reads(w["seed"], w["genome"], w["depth"], w["avg_len"], w["sd_len"], error_rate=w["error"], min_len=w["min_len"])
    e = elba_amd.Engine(w["k"], w["lower"], w["upper"])
    e.set_reads(packed, off, lens)
    e.count_kmers(); e.create_kmer_matrix(); e.create_seed_matrix()
    al = e.align_seeds()
    sg = e.transitive_reduction(0.65, 1000)
    e.generate_contigs()                                     # warm-up: buffers allocated
    runs = [e.generate_contigs() for _ in range(reps)]
    st = runs[-1]
    c = e.export_contigs()
    out_bytes = int(c["seq_off"][-1]) + 8 * 2 * (c["n"] + 1) + 13 * int(c["chain_off"][-1])
    e.close()
    ms = sorted(r["ms_total"] for r in runs)
    mr = sorted(r["ms_rank"] for r in runs)
    return {"workload": name, "params": w, "reads": int(len(lens)), "aligned_pairs": int(al["nalignments"]), "string_graph": {"nnz": int(sg["nnz"]), "ms_total": round(sg["ms_total"], 4)},
            "contig_stage": {"ms_total_median": round(ms[len(ms) // 2], 4), "ms_total_min": round(ms[0], 4), "ms_rank_median": round(mr[len(mr) // 2], 4), "reps": reps},
            "counts": {k: int(st[k]) for k in ("nreads", "branches", "components", "used_components", "contigs", "cycles", "contig_reads", "bases", "longest")},
            "output_bytes": {"seq": int(c["seq_off"][-1]), "all_exported": out_bytes}, "wall_s": round(time.time() - t0, 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--workload", choices=sorted(WORKLOADS), action="append")
    a = ap.parse_args()
    res = [run(n, WORKLOADS[n], a.reps) for n in (a.workload or sorted(WORKLOADS))]
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
