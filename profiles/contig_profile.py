"""Contig stage (elba_generate_contigs, contig.hip) on two workloads: reads -> B -> x-drop alignments -> string graph -> contigs on one GPU.
The stage is timed by its own device events (ms_total, ms_rank) on calls after a warm-up call; the string graph's stage time is recorded beside
it.  --flags F runs elba_generate_contigs_ex with F (1 circular contigs, 2 single-read contigs, 3 both) in place of the plain call;
--rings N adds a synthetic graph of N reads in cycles of 8 (loaded as an edge list), --chain N one of N reads in a single path (no cycle).
--clip-tips T clips tips of at most T reads (elba_clip_tips, 4 rounds) before the contigs and records the call's own times; the string graph
is rebuilt before every timed clip, since the call changes it.
Usage: python profiles/contig_profile.py OUT.json [--reps N] [--flags F] [--rings N] [--chain N] [--clip-tips T]"""
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


def _generate(e, flags):
    return e.generate_contigs() if flags is None else e.generate_contigs(circular=bool(flags & 1), singletons=bool(flags & 2))


def _synthetic(n, ring):
    """n reads of 32 bases under shuffled ids, chained in rings of `ring` reads (0: one path); every prefix 8 bases."""
    from elba_amd.capi import OVERLAP_DTYPE
    rng = np.random.default_rng(1)
    ids = rng.permutation(n).astype(np.int64)
    x, y = ids[:-1], ids[1:]
    if ring:
        keep = (np.arange(n - 1) % ring) != ring - 1
        x, y = np.concatenate([x[keep], ids[ring - 1::ring]]), np.concatenate([y[keep], ids[0::ring][:len(ids[ring - 1::ring])]])
    r, c = np.minimum(x, y), np.maximum(x, y)
    o = np.lexsort((c, r))
    v = np.zeros(len(r), dtype=OVERLAP_DTYPE)
    v["passed"] = 1; v["direction"] = 1; v["directionT"] = 2; v["suffix"] = 8; v["suffixT"] = 8
    lens = np.full(n, 32, dtype=np.uint32)
    return rng.integers(0, 256, 8 * n + 16).astype(np.uint8), (np.arange(n, dtype=np.uint64) * 8), lens, r[o], c[o], v


def run(name, w, reps, flags=None, clip=0):
    t0 = time.time()
    if "synthetic" in w:
        packed, off, lens, rows, cols, vals = _synthetic(w["synthetic"], w["ring"])
        e = elba_amd.Engine(17, 2, 8)
        e.set_reads(packed, off, lens)
        e.set_overlaps(len(lens), rows, cols, vals)
        al = {"nalignments": len(rows)}
        sg = e.transitive_reduction(0.0, 0)
    else:
        packed, off, lens, _ = elba_amd.synth_reads(w["seed"], w["genome"], w["depth"], w["avg_len"], w["sd_len"], error_rate=w["error"], min_len=w["min_len"])
        e = elba_amd.Engine(w["k"], w["lower"], w["upper"])
        e.set_reads(packed, off, lens)
        e.count_kmers(); e.create_kmer_matrix(); e.create_seed_matrix()
        al = e.align_seeds()
        sg = e.transitive_reduction(0.65, 1000)
    tips = None
    if clip:
        cutoff, fuzz = (0.0, 0) if "synthetic" in w else (0.65, 1000)
        clips = []
        for _ in range(reps + 1):                            # the first one is the warm-up
            clips.append(e.clip_tips(clip, 4))
            if len(clips) <= reps:
                e.transitive_reduction(cutoff, fuzz)
        mt = sorted(c["ms_total"] for c in clips[1:]); mc = sorted(c["ms_compact"] for c in clips[1:])
        tips = {"max_tip_reads": clip, "rounds": 4, "ms_total_median": round(mt[len(mt) // 2], 4), "ms_compact_median": round(mc[len(mc) // 2], 4),
                "counts": {k: int(clips[-1][k]) for k in ("nnz_before", "nnz_after", "dead_ends", "tips", "reads_removed", "spared_anchors", "rounds_run")}}
    _generate(e, flags)                                      # warm-up: buffers allocated
    runs = [_generate(e, flags) for _ in range(reps)]
    st = runs[-1]
    c = e.export_contigs()
    out_bytes = int(c["seq_off"][-1]) + 8 * 2 * (c["n"] + 1) + 13 * int(c["chain_off"][-1])
    e.close()
    ms = sorted(r["ms_total"] for r in runs)
    mr = sorted(r["ms_rank"] for r in runs)
    return {"workload": name, "flags": flags, "tip_stage": tips, "params": w, "reads": int(len(lens)), "aligned_pairs": int(al["nalignments"]), "string_graph": {"nnz": int(sg["nnz"]), "ms_total": round(sg["ms_total"], 4)},
            "contig_stage": {"ms_total_median": round(ms[len(ms) // 2], 4), "ms_total_min": round(ms[0], 4), "ms_total_max": round(ms[-1], 4), "ms_rank_median": round(mr[len(mr) // 2], 4),
                             "ms_rank_min": round(mr[0], 4), "ms_rank_max": round(mr[-1], 4), "reps": reps},
            "counts": {k: int(st[k]) for k in ("nreads", "branches", "components", "used_components", "contigs", "cycles", "contig_reads", "bases", "longest")},
            "output_bytes": {"seq": int(c["seq_off"][-1]), "all_exported": out_bytes}, "wall_s": round(time.time() - t0, 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--workload", choices=sorted(WORKLOADS), action="append")
    ap.add_argument("--flags", type=int, choices=[0, 1, 2, 3])
    ap.add_argument("--rings", type=int, default=0)
    ap.add_argument("--chain", type=int, default=0)
    ap.add_argument("--clip-tips", type=int, default=0)
    a = ap.parse_args()
    res = [] if (a.rings or a.chain) and not a.workload else [run(n, WORKLOADS[n], a.reps, a.flags, a.clip_tips) for n in (a.workload or sorted(WORKLOADS))]
    if a.rings:
        res.append(run("rings-of-8", {"synthetic": a.rings, "ring": 8}, a.reps, a.flags, a.clip_tips))
    if a.chain:
        res.append(run("one-path", {"synthetic": a.chain, "ring": 0}, a.reps, a.flags, a.clip_tips))
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
