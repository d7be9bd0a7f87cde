"""elba_place_reads (place.hip) on the benchmark's workloads: reads -> k-mers -> B -> alignments -> string graph -> cleaning -> contigs, then
the placement call --reps + --warmup times; the first --warmup calls are dropped and the median (min, max) of the others' own device events
(ms_total) is reported beside the counts, the byte model of place.hip's header, and elba_read_pileup's ms_total on the same pairs for scale
(median of as many calls; measured last, because it is no export).  A progress line goes to stderr after every stage.
--bad-read-cutoff is the reduction's (0.65 in the reference; at 15 % error it flags nearly every read of the default workload, which the
default skip mask then leaves out: 0 keeps them); several values are run one after another on the same alignments.
Usage: python profiles/place_profile.py OUT.json [--workload NAME] [--reps 15] [--warmup 3] [--bad-read-cutoff 0.65 [0 ...]] [--skip-flags 1]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import elba_amd  # noqa: E402
from bench import WORKLOADS  # noqa: E402

COUNTS = ("nreads", "chain", "anchored", "unanchored", "skipped", "empty", "candidates", "clipped", "outside", "wrapped", "segments", "max_depth", "credited_bases")


def _say(t0, what):
    print("[%7.1f s] %s" % (time.time() - t0, what), file=sys.stderr, flush=True)


def _mmm(xs):
    xs = sorted(xs)
    return [round(xs[len(xs) // 2], 4), round(xs[0], 4), round(xs[-1], 4)]


def byte_model(npairs, st, ncontigs, key_bits):
    """Algorithmic bytes of one call, as place.hip's header counts them."""
    M, E = st["nreads"], 2 * (st["chain"] + st["anchored"] - st["outside"] + st["wrapped"])
    passes = (key_bits + 7) // 8
    parts = {"pairs_read": 52 * npairs, "pair_lookups": 9 * npairs, "candidate_atomics": 8 * st["candidates"], "chain_elements": 17 * st["chain"],
             "records_written_and_read": 2 * 24 * M, "anchor_pairs": 36 * st["anchored"], "endpoints_written": 8 * E, "sort": 2 * 8 * E * passes,
             "marks_scans_groups_tokens": 14 * 4 * E, "credits": 8 * E, "segments_written": 8 * st["segments"] + 8 * ncontigs}
    parts["total"] = sum(parts.values())
    return parts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out")
    ap.add_argument("--workload", default="200k-long-reads", choices=sorted(WORKLOADS))
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--bad-read-cutoff", type=float, nargs="+", default=[0.65])
    ap.add_argument("--skip-flags", type=int, default=1)
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
    npairs = int(al["nalignments"])
    res = []
    for cutoff in a.bad_read_cutoff:
        sg = e.transitive_reduction(cutoff, 1000)
        e.simplify_graph(4, 8)
        cs = e.generate_contigs(circular=True, singletons=True)
        _say(t0, "cutoff %g: S has %d entries, %d contigs of %d chain reads" % (cutoff, sg["nnz"], cs["contigs"], cs["contig_reads"]))
        runs = [e.place_reads(a.skip_flags)[1] for _ in range(a.warmup + a.reps)][a.warmup:]
        st = runs[-1]
        _say(t0, "placed: %s" % {k: st[k] for k in COUNTS})
        key_bits = 1 + int(cs["longest"]).bit_length() + max(1, int(cs["contigs"]).bit_length())
        model = byte_model(npairs, st, int(cs["contigs"]), key_bits)
        ms = _mmm([r["ms_total"] for r in runs])
        res.append(dict(workload=a.workload, bad_read_cutoff=cutoff, skip_flags=a.skip_flags, passed_pairs=int(al["passed"]), reads=int(len(lens)), pairs=npairs,
                        string_nnz=int(sg["nnz"]), contigs=int(cs["contigs"]), longest_contig=int(cs["longest"]), key_bits=key_bits, counts={k: int(st[k]) for k in COUNTS},
                        place_ms_total_median_min_max=ms, reps=a.reps, warmup=a.warmup, byte_model=model, model_gb_per_s_at_median=round(model["total"] / ms[0] / 1e6, 1)))
    pile = [e.read_pileup(mode=0, margin=0, min_depth=1, min_run=1, trim_len=2500) for _ in range(a.warmup + a.reps)][a.warmup:]
    _say(t0, "pileup: %d intervals" % pile[-1]["intervals"])
    for r in res:
        r.update(read_pileup_ms_total_median_min_max=_mmm([p["ms_total"] for p in pile]), read_pileup_intervals=int(pile[-1]["intervals"]), read_pileup_segments=int(pile[-1]["segments"]))
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))
    e.close()


if __name__ == "__main__":
    main()
