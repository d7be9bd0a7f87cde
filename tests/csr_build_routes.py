"""The cases of tests/test_gpu_csr_build_routes.py and of its recorder (tests/golden/record_csr_build_routes.py): one per route through the CSR build of A
(csrc/matrix.hip, finish_matrix_from_sorted_csc) — the k-mer stage's sort path and its bucket kernels, with and without hints and inline partners, the pair
sort, the sort that does not write the rows, dense matrices, positions beyond 16 bits, a rebuild from a consumed hand-off, device and host triples, a shard's
panel, and degenerate shapes.  run_case() returns what the fixture holds of a case: the format counters, the sizes, SHA-256 digests of A in both
orientations and, after one create_seed_matrix, of B (a panel with inline partners is multiplied through the mirror exchange only: no B).  Under gather
slots the id field of a row entry that fetches its column names a slot, and which slot depends on scheduling: such entries are mapped through a_slot_kid
before they are hashed."""
import functools
import hashlib

import numpy as np

import elba_amd
import gpu_util as gu
import kmer_stage_routes as ksr

STATS = ("matrix_hints", "matrix_inline", "matrix_suffix", "matrix_csr_words", "matrix_pos16", "matrix_fbits", "matrix_col_stride", "padded_columns", "triples_path")
CSR_INLINE = 3      # ELBA_CSR_INLINE of include/elba_amd.h


def _sha(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def _record(e, ms, rows=None, multiply=True):
    """rows: (lo, hi) of a windowed matrix (B is exported for them); multiply False: a panel with inline partners, which only the mirror exchange multiplies"""
    rec = {s: int(e.get_stat(s)) for s in STATS}
    rec["gather_slots"] = int(e.get_stat("gather_slots") > 0)
    rec["slots_compact"] = int(e.device_view()["a_gather_slots"] > 0)      # (the padded store holds the columns still fetched: ids of row entries are slots)
    rec.update({f: int(ms[f]) for f in ("nrows", "ncols", "nnz", "max_row_nnz")})
    v = e.device_view()
    M, N, Z = int(v["M"]), int(v["N"]), int(v["Z"])
    csr = gu.host_copy(v["a_csr"], Z, np.uint64)
    if v["a_slot_kid"] and v["a_gather_slots"] > 0:
        slot_kid = gu.host_copy(v["a_slot_kid"], v["a_gather_slots"], np.uint32).astype(np.uint64)
        assert v["a_csr_format"] == CSR_INLINE
        named = ((csr >> np.uint64(63)) == 0) & (((csr >> np.uint64(30)) & np.uint64(3)) == 0)      # (an entry that fetches its column: include/elba_amd.h, a_gather_slots)
        csr[named] =(slot_kid[(csr[named] >> np.uint64(32)).astype(np.int64)] << np.uint64(32)) | (csr[named] & np.uint64(0xFFFFFFFF))
    rec.update(a_colptr=_sha(gu.host_copy(v["a_colptr"], N + 1, np.uint32)), a_csc=_sha(gu.host_copy(v["a_csc"], Z, np.uint64)),
               a_rowptr=_sha(gu.host_copy(v["a_rowptr"], M + 1, np.uint32)), a_csr=_sha(csr))
    if multiply:
        st = e.create_seed_matrix()
        B = e.export_csr(*rows) if rows else e.export_csr()
        rec.update(b_nnz=int(st["nnz"]), b_csr=_sha(B["rowptr"], B["col"], B["val"]))
    return rec


@functools.lru_cache(maxsize=None)
def read_set(name):
    if name == "dense":          # tests/test_gpu_parity.py, test_dense_columns_take_the_path_of_their_own
        return elba_amd.synth_reads(91, 60000, 30, 3000, 600, error_rate=0.01, min_len=500, repeat_families=3, repeat_fraction=0.1, repeat_len=400)[:3]
    if name == "long":           # tests/test_gpu_parity.py, test_reads_longer_than_16_bit_positions_use_the_lookup_path
        packed, off, lens, base = [], [], [], 0
        for p, o, l, _ in (elba_amd.synth_reads(54, 90000, 6, 3000, 500, error_rate=0.05, min_len=500), elba_amd.synth_reads(53, 90000, 6, 70000, 4000, error_rate=0.05, min_len=66000)):
            nb = int(o[-1]) + (int(l[-1]) + 3) // 4
            packed.append(p[:nb]); off.append(o + np.uint64(base)); lens.append(l); base += nb
        return np.concatenate(packed + [np.zeros(16, np.uint8)]), np.concatenate(off), np.concatenate(lens)
    return ksr.read_set(name)


SORT, MSD = {"kmer_no_msd": 1}, {"kmer_msd": 1}
# name -> (reads, k, lower, upper, options)
READS_CASES = {
    "sort": ("r17", 17, 2, 8, SORT),
    "msd": ("r17", 17, 2, 8, MSD),
    "sort_no_inline": ("r17", 17, 2, 8, dict(SORT, no_inline=1)),
    "msd_no_inline": ("r17", 17, 2, 8, dict(MSD, no_inline=1)),
    "sort_no_hints": ("r17", 17, 2, 8, dict(SORT, no_hints=1)),
    "msd_no_hints": ("r17", 17, 2, 8, dict(MSD, no_hints=1)),
    "sort_csr_pairs": ("r17", 17, 2, 8, dict(SORT, csr_pairs=1)),
    "msd_csr_pairs": ("r17", 17, 2, 8, dict(MSD, csr_pairs=1)),
    "sort_tune1": ("r17", 17, 2, 8, dict(SORT, tune1=1)),
    "dense": ("dense", 17, 2, 40, {}),
    "dense_msd": ("dense", 17, 2, 40, MSD),
    "dense_msd_pairs_late": ("dense", 17, 2, 40, dict(MSD, csr_pairs_late=1)),
    "dense_no_suffix": ("dense", 17, 2, 40, {"no_suffix": 1}),
    "long_positions": ("long", 17, 2, 30, {}),
}
REBUILD_CASES = {"rebuild_sort": SORT, "rebuild_msd": MSD}
# name -> (source of the triples, options of the engine that takes them, device triples?)
TRIPLES_CASES = {
    "triples_msd": ("triples", MSD, True),
    "triples_sorted": ("triples_empty_column", MSD, True),
    "triples_sorted_csr_pairs": ("triples_empty_column", dict(MSD, csr_pairs=1), True),
    "triples_host": ("triples", {}, False),
}
# name -> (reads, k, lower, upper, panel_inline)
PANEL_CASES = {
    "panel": ("r17", 17, 2, 8, 0),
    "panel_inline": ("r17", 17, 2, 8, 1),
    "panel_dense": ("dense", 17, 2, 40, 0),
}
# name -> (M, N, rows, cols, vals)
SHAPE_CASES = {
    "no_entries": (5, 3, [], [], []),
    "one_row": (1, 4, [0, 0, 0], [0, 2, 3], [7, 1, 4]),
    "one_column": (6, 1, [0, 2, 5], [0, 0, 0], [3, 9, 2]),
}
ALL_CASES = tuple(READS_CASES) + tuple(REBUILD_CASES) + tuple(TRIPLES_CASES) + tuple(PANEL_CASES) + tuple(SHAPE_CASES)


def _engine(reads, k, lo, up, opts):
    e = elba_amd.Engine(k, lo, up, options=dict(opts))
    e.set_reads(*read_set(reads))
    e.count_kmers()
    return e


def _reads_case(name):
    e = _engine(*READS_CASES[name])
    rec = _record(e, e.create_kmer_matrix())
    e.close()
    return rec


def _rebuild(name):
    """create_kmer_matrix three times after ONE count_kmers: from the hand-off, from the consumed hand-off, and after release_workspace"""
    e = _engine("r17", 17, 2, 8, REBUILD_CASES[name])
    recs = [_record(e, e.create_kmer_matrix()), _record(e, e.create_kmer_matrix())]
    e.release_workspace()
    recs.append(_record(e, e.create_kmer_matrix()))
    e.close()
    return recs


@functools.lru_cache(maxsize=None)
def _matrix(reads, k, lo, up):
    """A of a read set as host triples (M, N, rows, cols, vals), in column order"""
    e = _engine(reads, k, lo, up, {})
    e.create_kmer_matrix()
    A = e.export_kmer_matrix()
    e.close()
    cols = np.repeat(np.arange(A["N"], dtype=np.int64), np.diff(A["colptr"]))
    return int(A["M"]), int(A["N"]), A["csc_read"].astype(np.int64), cols, A["csc_pos"].astype(np.uint32)


def _triples(name):
    import torch
    source, opts, device = TRIPLES_CASES[name]
    M, N, rows, cols, vals = _matrix("r17", 17, 2, 8)
    perm = np.random.default_rng(5).permutation(len(rows))
    rows, cols, vals = rows[perm], cols[perm], vals[perm]
    if source == "triples_empty_column":
        keep = cols != cols[0]
        rows, cols, vals = rows[keep], cols[keep], vals[keep]
    e = elba_amd.Engine(17, 2, 8, options=dict(opts))
    if device:
        dr, dc, dv = (torch.from_numpy(np.ascontiguousarray(a)).to("cuda") for a in (rows, cols, vals.astype(np.int32)))
        ms = e.set_kmer_matrix_device(M, N, len(rows), dr.data_ptr(), dc.data_ptr(), dv.data_ptr())
    else:
        ms = e.set_kmer_matrix(M, N, rows, cols, vals)
    rec = _record(e, ms)
    e.close()
    return rec


def _panel(name):
    """Rank 1 of two simulated ranks on one GPU: its panel is every column that reaches one of its rows, whole, as records (column id, read << 32 | pos),
    a column's entries contiguous and in (read, pos) order — what tests/dist_step_cases.py hands elba_dist_set_panel"""
    import torch
    from elba_amd.distributed import HipBackend
    reads, k, lo, up, inline = PANEL_CASES[name]
    M, N, rows, cols, vals = _matrix(reads, k, lo, up)
    row_lo, row_hi = M // 2, M
    keep = np.isin(cols, np.unique(cols[(rows >= row_lo) & (rows < row_hi)]))
    r, c, v = rows[keep], cols[keep], vals[keep].astype(np.int64)
    order = np.lexsort((v, r, c))
    rec = torch.from_numpy(np.ascontiguousarray(np.stack([c[order], (r[order] << 32) | v[order]], axis=1).astype(np.int64))).to("cuda")
    be = HipBackend(k, lo, up, 0)
    be.set_option("panel_inline", inline)
    ms = be.set_panel(rec, M, N, row_lo, row_hi)
    out = _record(be.e, ms, rows=(row_lo, row_hi), multiply=not inline)
    be.e.close()
    return out


def _shape(name):
    M, N, rows, cols, vals = SHAPE_CASES[name]
    e = elba_amd.Engine(17, 2, 8)
    rec = _record(e, e.set_kmer_matrix(M, N, np.asarray(rows, dtype=np.int64), np.asarray(cols, dtype=np.int64), np.asarray(vals, dtype=np.uint32)))
    e.close()
    return rec


def run_case(name):
    """The record of one case (a list of three for the rebuild cases)."""
    for cases, run in ((READS_CASES, _reads_case), (REBUILD_CASES, _rebuild), (TRIPLES_CASES, _triples), (PANEL_CASES, _panel), (SHAPE_CASES, _shape)):
        if name in cases:
            return run(name)
    raise KeyError(name)
