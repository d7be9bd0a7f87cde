"""elba_polish_contigs (polish.hip) on the benchmark's workloads: reads -> k-mers -> B -> alignments -> string graph -> cleaning -> contigs,
then the polishing call --reps + --warmup times; the first --warmup calls are dropped and the median (min, max) of the others' own device
events (ms_total, ms_align) is reported beside the counts, the cells (the sum of n * W over the voters), the bytes of the choices
(cells / 4) and elba_place_reads' ms_total on the same input (median of as many calls).  ms_total - ms_align holds the shared placement
pass, the backward walks with their atomics, the calls and the write.  A progress line goes to stderr after every stage.
Usage: python profiles/polish_profile.py OUT.json [--workload NAME] [--reps 15] [--warmup 3] [--bad-read-cutoff 0] [--band 64]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import elba_amd  # noqa: E402
from bench import WORKLOADS  # noqa: E402

COUNTS = ("nreads", "voted", "rejected", "outside", "low_depth_columns", "bases_before", "bases_after", "sum_dist", "cells", "batches")


def _say(t0, what):
    print("[%7.1f s] %s" % (time.time() - t0, what), file=sys.stderr, flush=True)


def _mmm(xs):
    xs = sorted(xs)
    return [round(xs[len(xs) // 2], 4), round(xs[0], 4), round(xs[-1], 4)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out")
    ap.add_argument("--workload", default="200k-long-reads", choices=sorted(WORKLOADS))
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--bad-read-cutoff", type=float, nargs="+", default=[0.0])
    ap.add_argument("--band", type=int, nargs="+", default=[64])
    ap.add_argument("--max-diff", type=float, default=0.25)
    ap.add_argument("--min-depth", type=int, default=3)
    a = ap.parse_args()
    w = WORKLOADS[a.workload]
    t0 = time.time()
    rep = w.get("repeats", (0, 0.0, 0))
    packed, off, lens, _ = elba_amd.synth_reads(w["seed"], w["genome"], w["depth"], w["avg_len"], w["sd_len"], error_rate=w["error"], min_len=w["min_len"],
                                                repeat_families=rep[0], repeat_fraction=rep[1], repeat_len=rep[2])
    _say(t0, "%d reads generated" % len(lens))
    e = elba_amd.Engine(w["k"], w["lower"], w["upper"])
    e.set_reads(packed, off, lens)
    e.count_kmers(); e.create_kmer_matrix()
    ov = e.create_seed_matrix()
    _say(t0, "B has %d entries" % ov["nnz"])
    al = e.align_seeds()
    _say(t0, "%d pairs aligned, %d passed, %.0f ms" % (al["nalignments"], al["passed"], al["ms_total"]))
    res = []
    for cutoff in a.bad_read_cutoff:
        sg = e.transitive_reduction(cutoff, 1000)
        e.simplify_graph(4, 8)
        cs = e.generate_contigs(circular=True, singletons=True)
        _say(t0, "cutoff %g: S has %d entries, %d contigs of %d chain reads" % (cutoff, sg["nnz"], cs["contigs"], cs["contig_reads"]))
        place = [e.place_reads(1)[1] for _ in range(a.warmup + a.reps)][a.warmup:]
        for band in a.band:
            runs = [e.polish_contigs(1, band, a.max_diff, a.min_depth)[1] for _ in range(a.warmup + a.reps)][a.warmup:]
            st = runs[-1]
            _say(t0, "band %d: %s" % (band, {k: st[k] for k in COUNTS}))
            tot, aln = _mmm([r["ms_total"] for r in runs]), _mmm([r["ms_align"] for r in runs])
            res.append(dict(workload=a.workload, bad_read_cutoff=cutoff, band=band, max_diff=a.max_diff, min_depth=a.min_depth, reads=int(len(lens)), pairs=int(al["nalignments"]),
                            contigs=int(cs["contigs"]), longest_contig=int(cs["longest"]), counts={k: int(st[k]) for k in COUNTS}, trace_bytes=int(st["cells"]) // 4,
                            polish_ms_total_median_min_max=tot, polish_ms_align_median_min_max=aln, ms_outside_the_align_kernel_at_median=round(tot[0] - aln[0], 4),
                            gcells_per_s_align_at_median=round(st["cells"] / aln[0] / 1e6, 2) if aln[0] > 0 else None,
                            place_ms_total_median_min_max=_mmm([p["ms_total"] for p in place]), reps=a.reps, warmup=a.warmup))
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))
    e.close()


if __name__ == "__main__":
    main()
