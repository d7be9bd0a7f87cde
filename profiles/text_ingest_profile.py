"""Text ingest (elba_set_reads_text, text_index.hip) on the read set bench.py's ingest() builds (one record per read, the whole read on one
line, names ">%d"), beside what it replaces: the host's index (fasta.write_fai + read_fai, wall time) followed by elba_set_reads_fasta.
Times of the two calls are their own device events (ms_total spans the H2D copy of the chunk to the last D2H), medians of --reps calls after
one warm-up call each; the packed bytes of the two paths are compared.  Index bytes: the chunk twice plus the side arrays, as DESIGN.md
§4.18 counts them (12 B per tile, 36 B per line, 72 B per record for FASTA).
Usage: python profiles/text_ingest_profile.py OUT.json [--workload NAME] [--reps N]"""
import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

import bench  # noqa: E402
import elba_amd  # noqa: E402
from elba_amd import fasta  # noqa: E402

PEAK_BS = bench.PEAK_GBS * 1e9


def fasta_of(packed, off, lens):
    letters = np.frombuffer(b"ACGT", dtype=np.uint8)
    nb = (lens.astype(np.int64) + 3) // 4
    parts = []
    for r in range(len(lens)):
        by = packed[int(off[r]):int(off[r]) + int(nb[r])]
        codes = np.stack([(by >> 6) & 3, (by >> 4) & 3, (by >> 2) & 3, by & 3], axis=1).reshape(-1)[:int(lens[r])]
        parts.append(b">%d\n" % r); parts.append(letters[codes].tobytes()); parts.append(b"\n")
    return b"".join(parts)


def med(x):
    x = sorted(x)
    return round(float(x[len(x) // 2]), 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out")
    ap.add_argument("--workload", default="200k-long-reads", choices=sorted(bench.WORKLOADS))
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    w = bench.WORKLOADS[a.workload]
    rep = w.get("repeats", (0, 0.0, 0))
    packed, off, lens, _ = elba_amd.synth_reads(w["seed"], w["genome"], w["depth"], w["avg_len"], w["sd_len"], error_rate=w["error"], min_len=w["min_len"],
                                                repeat_families=rep[0], repeat_fraction=rep[1], repeat_len=rep[2])
    chunk = fasta_of(packed, off, lens)
    out = {"workload": a.workload, "reads": int(len(lens)), "chunk_bytes": len(chunk), "reps": a.reps}
    # what the text call replaces: the host's index, then elba_set_reads_fasta
    with tempfile.TemporaryDirectory() as d:
        p = os.path.join(d, "reads.fa")
        with open(p, "wb") as f:
            f.write(chunk)
        t0 = time.perf_counter()
        fasta.write_fai(p)
        _, recs = fasta.read_fai(p + ".fai")
        out["host_index_wall_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
    e = elba_amd.Engine(w["k"], w["lower"], w["upper"])
    e.set_reads_fasta(chunk, 0, recs)
    runs = [e.set_reads_fasta(chunk, 0, recs) for _ in range(a.reps)]
    out["set_reads_fasta"] = {"ms_total": med([r["ms_total"] for r in runs]), "ms_encode": med([r["ms_encode"] for r in runs])}
    ref = e.export_reads(len(lens), runs[-1]["packed_bytes"])
    e.close()
    e = elba_amd.Engine(w["k"], w["lower"], w["upper"])
    e.set_reads_text(chunk)
    runs = [e.set_reads_text(chunk) for _ in range(a.reps)]
    st = runs[-1]
    got = e.export_reads(st["nreads"], st["packed_bytes"])
    _, trecs = e.export_read_index()
    e.close()
    out["same_reads_and_records"] = bool(all((x == y).all() for x, y in zip(ref, got)) and (trecs == recs).all())
    ms_index, ms_encode = med([r["ms_index"] for r in runs]), med([r["ms_encode"] for r in runs])
    ntiles = (len(chunk) + 4095) // 4096
    index_bytes = 2 * len(chunk) + 12 * ntiles + 36 * st["lines"] + 72 * st["nreads"]
    encode_bytes = len(chunk) + st["packed_bytes"]
    out["set_reads_text"] = {"ms_total": med([r["ms_total"] for r in runs]), "ms_index": ms_index, "ms_encode": ms_encode, "lines": int(st["lines"]),
                             "index_bytes": int(index_bytes), "index_frac_of_hbm_peak": round(index_bytes / (ms_index * 1e-3) / PEAK_BS, 4),
                             "encode_bytes": int(encode_bytes), "encode_frac_of_hbm_peak": round(encode_bytes / (ms_encode * 1e-3) / PEAK_BS, 4)}
    out["replaced_ms"] = round(out["host_index_wall_ms"] + out["set_reads_fasta"]["ms_total"], 1)
    line = json.dumps(out)
    print(line)
    with open(a.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
