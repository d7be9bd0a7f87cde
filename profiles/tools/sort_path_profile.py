"""Times elba_count_kmers on the k-mer stage's SORT path (csrc/kmer.hip): per input the device times of the call (ms_total, ms_count, ms_sort) and its
wall time, the median and the range of --reps calls after one warm-up call, one JSON line per input.  The inputs: the reads of BASELINE configs[3]
(40x, 15 kb, 0.5 % error) on a genome of --genome bases at k = 63 in one pass, the same in value-range passes (kmer_batch_instances = I // 4 + 1), and
at k = 17 with the partition switched off (kmer_no_msd).  Another build of the library is compared by running this script in a process of its own with
ELBA_AMD_LIB set:  python profiles/tools/sort_path_profile.py [--genome 2500000] [--reps 5] [--label NAME]"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

import numpy as np      # noqa: E402

import elba_amd      # noqa: E402


def measure(label, name, reads, k, lo, up, options, reps):
    e = elba_amd.Engine(k, lo, up, options=options)
    e.set_reads(*reads)
    e.count_kmers()
    rows = []
    for _ in range(reps):
        t0 = time.perf_counter()
        ks = e.count_kmers()
        rows.append((ks["ms_total"], ks["ms_count"], ks["ms_sort"], (time.perf_counter() - t0) * 1e3))
    out = {"label": label, "input": name, "k": k, "instances": int(ks["instances"]), "reliable": int(ks["reliable"]), "entries": int(ks["entries"]),
           "kmer_path": int(e.get_stat("kmer_path")), "kmer_passes": int(e.get_stat("kmer_passes")), "reps": reps}
    for i, f in enumerate(("ms_total", "ms_count", "ms_sort", "wall_ms")):
        v = [r[i] for r in rows]
        out[f] = round(statistics.median(v), 3)
        out[f + "_range"] = [round(min(v), 3), round(max(v), 3)]
    e.close()
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--genome", type=int, default=2500000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--label", default=os.path.basename(os.environ.get("ELBA_AMD_LIB", "tree")))
    a = ap.parse_args()
    packed, off, lens, _ = elba_amd.synth_reads(3, a.genome, 40.0, 15000.0, 2000.0, error_rate=0.005, min_len=1000)
    reads = (packed, off, lens)
    I63 = int(np.maximum(lens.astype(np.int64) - 62, 0).sum())
    measure(a.label, "k63_one_pass", reads, 63, 2, 4, None, a.reps)
    measure(a.label, "k63_four_passes", reads, 63, 2, 4, {"kmer_batch_instances": I63 // 4 + 1}, a.reps)
    measure(a.label, "k17_no_msd", reads, 17, 2, 4, {"kmer_no_msd": 1}, a.reps)


if __name__ == "__main__":
    main()
