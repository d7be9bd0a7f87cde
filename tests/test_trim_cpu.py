"""CPU: the numpy restatement of elba_trim_reads (trim_util.py) against a brute-force version on ASCII strings; the new symbols in the
built library and the header; k_trim_repack's register notes in the gfx950 code object."""
import ctypes
import os
import re

import numpy as np

import contig_util as cu
import trim_util as tu
from oracle import pyoracle as po
from test_kernel_resources_cpu import LIB, _kernel_notes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("elba_trim_reads", "elba_export_trim_map", "elba_free_trim_map", "elba_get_trimmed_reads_device", "elba_adopt_trimmed_reads")


def _small_case(rng):
    M = int(rng.integers(1, 9))
    seqs = cu.random_reads(rng, M, lo=1, hi=70)
    if rng.random() < 0.3:
        seqs[int(rng.integers(0, M))] = ""                        # a read of length 0
    lens = np.array([len(s) for s in seqs], np.int64)
    pairs = [(a, b) for a in range(M) for b in range(a + 1, M) if rng.random() < 0.7]
    for _ in range(int(rng.integers(0, 4))):                      # the same pair more than once: deeper pileups, more runs
        if pairs:
            pairs.append(pairs[int(rng.integers(0, len(pairs)))])
    pairs.sort()
    rows = np.array([p[0] for p in pairs], np.int64); cols = np.array([p[1] for p in pairs], np.int64)
    vals = np.zeros(len(pairs), po.OVERLAP_DTYPE)
    for f0, f1, who in (("begQ", "endQ", rows), ("begT", "endT", cols)):
        L = lens[who]
        x = np.sort(np.stack([rng.integers(0, L + 1), rng.integers(0, L + 1)], 1), 1) if len(pairs) else np.zeros((0, 2), np.int64)
        vals[f0], vals[f1] = x[:, 0], x[:, 1]
    vals["passed"] = rng.integers(0, 2, len(pairs)); vals["score"] = rng.integers(-1, 30, len(pairs))
    cfg = dict(mode=int(rng.integers(0, 2)), margin=int(rng.integers(0, 4)), min_depth=int(rng.integers(1, 4)), min_run=int(rng.integers(1, 12)),
               trim_len=int(rng.integers(0, 20)))
    return seqs, lens, rows, cols, vals, cfg


def test_restatement_equals_brute_force_on_strings():
    rng = np.random.default_rng(4242)
    pieces_seen = splits_seen = 0
    for case in range(300):
        seqs, lens, rows, cols, vals, cfg = _small_case(rng)
        packed, off, _ = cu.pack(seqs)
        # the source's own padding bits are garbage: the restatement must not let them through
        garbage = packed.copy()
        for o, L in zip(off, lens):
            if L % 4:
                garbage[int(o) + int(L) // 4] |= int(rng.integers(0, 256)) & (0xff >> (2 * (int(L) % 4)))
        for mode in (0, 1):
            for min_len in (1, int(rng.integers(2, 20))):
                want_map, want_strs = tu.brute_force(seqs, rows, cols, vals, cfg, mode, min_len)
                got, st = tu.trim(garbage, off, lens, rows, cols, vals, cfg, mode=mode, min_len=min_len)
                assert list(zip(got["src_read"].tolist(), got["src_beg"].tolist(), got["src_end"].tolist())) == want_map, (case, mode, min_len)
                wp, wo, wl = cu.pack(want_strs)
                assert (got["len"] == wl).all() and (got["byte_off"] == wo).all(), (case, mode, min_len)
                assert got["packed"].shape == wp.shape and (got["packed"] == wp).all(), (case, mode, min_len)
                assert cu.seqs_of(got["packed"], got["byte_off"], got["len"]) == want_strs
                per = np.bincount(got["src_read"], minlength=len(seqs))
                assert st["pieces"] == len(want_map) and st["bases_out"] == sum(len(s) for s in want_strs) and st["bases_in"] == int(lens.sum())
                assert st["reads_dropped"] == int((per == 0).sum()) and st["reads_split"] == int((per >= 2).sum())
                assert st["reads_unchanged"] == sum(1 for v, a, b in want_map if per[v] == 1 and a == 0 and b == lens[v])
                assert st["longest"] == max([len(s) for s in want_strs], default=0) and st["packed_bytes"] == len(wp) - 16
                if mode == 1 and min_len == 1:
                    # the pieces are the runs the flags count: bit 0 <=> no piece, bit 1 <=> two or more
                    assert ((got["flags"] & 1) != 0).tolist() == (per == 0).tolist(), case
                    assert ((got["flags"] & 2) != 0).tolist() == (per >= 2).tolist(), case
                pieces_seen += len(want_map); splits_seen += int((per >= 2).sum())
    assert pieces_seen > 1000 and splits_seen > 50                   # the cases are not all empty


def test_library_exports_the_trim_symbols_and_the_abi_version_stays():
    assert os.path.exists(LIB), "library not built"
    L = ctypes.CDLL(LIB)
    for name in NEW_SYMBOLS:
        assert hasattr(L, name), name
    L.elba_abi_version.restype = ctypes.c_int
    assert L.elba_abi_version() == 3
    header = open(os.path.join(ROOT, "include", "elba_amd.h")).read()
    for name in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(elba_" % name, header), name
    for name in ("elba_trim_cfg", "elba_trim_stats", "elba_trim_map_t"):
        assert re.search(r"\}\s*%s;" % name, header), name
    assert re.search(r"#define\s+ELBA_ABI_VERSION\s+3\b", header)
    from elba_amd.capi import EXPORTED_SYMBOLS
    assert set(NEW_SYMBOLS) <= set(EXPORTED_SYMBOLS)


def test_repack_kernel_uses_no_scratch_and_spills_no_vgprs():
    notes = _kernel_notes()
    hits = [v for k, v in notes.items() if "k_trim_repack" in k]
    assert len(hits) == 1, len(hits)
    k = hits[0]
    assert k["private_segment_fixed_size"] == 0, k
    assert k["vgpr_spill_count"] == 0, k
    assert k["sgpr_spill_count"] == 0, k
    assert k["vgpr_count"] <= 64, k                                 # eight waves per SIMD: a streaming kernel hides its loads by occupancy
