"""ctypes binding of include/elba_amd.h and include/elba_synth.h (no torch types cross this boundary)."""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))


def lib_path():
    # ELBA_AMD_LIB: another build of the same library (A/B runs of kernel variants); never a different implementation
    return os.environ.get("ELBA_AMD_LIB") or os.path.join(_HERE, "lib", "libelba_amd.so")


def numeric_source_fingerprint():
    """sha256 (16 hex digits) of the sources that decide what the SpGEMM's numeric kernels do and what they read: the kernels themselves and
    the files that write the format of A (inline partners, hints, padded-column strides).  A rocprof counter summary under profiles/ is valid
    for exactly these sources: bench.py quotes `roofline.traffic` from profiles/traffic.json only while this matches the value stored there.
    None when the sources are not beside the library (an install without csrc/): nothing is quoted then."""
    import hashlib
    h = hashlib.sha256()
    try:
        for name in ("spgemm.hip", "spgemm_direct.hpp", "spgemm_table.hpp", "matrix.hip", "kmer_msd.hip", "kmer.hip", "common.hpp"):
            with open(os.path.join(_HERE, "csrc", name), "rb") as f:
                h.update(f.read())
    except OSError:
        return None
    return h.hexdigest()[:16]


ELBA_ERR_HIP = 3


class ElbaError(RuntimeError):
    def __init__(self, status, text):
        super().__init__("elba status %d: %s" % (status, text))
        self.status = status


class Seed(C.Structure):
    _fields_ = [("q0", C.c_uint32), ("t0", C.c_uint32), ("q1", C.c_uint32), ("t1", C.c_uint32), ("numshared", C.c_int32)]


SEED_DTYPE = np.dtype([("q0", "<u4"), ("t0", "<u4"), ("q1", "<u4"), ("t1", "<u4"), ("numshared", "<i4")])


class Cfg(C.Structure):
    _fields_ = [("k", C.c_int32), ("lower", C.c_int32), ("upper", C.c_int32), ("device", C.c_int32),
                ("workspace_hint_bytes", C.c_int64), ("flags", C.c_int32), ("timing_stride", C.c_int32)]


class KmerStats(C.Structure):
    _fields_ = [("nreads", C.c_int64), ("instances", C.c_int64), ("distinct", C.c_int64), ("reliable", C.c_int64), ("entries", C.c_int64),
                ("ms_total", C.c_float), ("ms_count", C.c_float), ("ms_lookup", C.c_float), ("ms_sort", C.c_float)]


class MatrixStats(C.Structure):
    _fields_ = [("nrows", C.c_int64), ("ncols", C.c_int64), ("nnz", C.c_int64), ("max_row_nnz", C.c_int64), ("ms_total", C.c_float)]


class OverlapStats(C.Structure):
    _fields_ = [("nrows", C.c_int64), ("products", C.c_int64), ("nnz_before_prune", C.c_int64), ("nnz", C.c_int64), ("nnz_diag", C.c_int64),
                ("nnz_upper", C.c_int64), ("max_numshared", C.c_int64), ("rows_lds", C.c_int64), ("rows_global", C.c_int64), ("rows_escalated", C.c_int64),
                ("algorithmic_bytes", C.c_int64), ("passes", C.c_int32), ("timed", C.c_int32),
                ("ms_total", C.c_float), ("ms_symbolic", C.c_float), ("ms_numeric", C.c_float), ("ms_finalize", C.c_float)]


class IngestStats(C.Structure):
    _fields_ = [("nreads", C.c_int64), ("bases", C.c_int64), ("packed_bytes", C.c_int64), ("chunk_bytes", C.c_int64), ("ms_total", C.c_float), ("ms_encode", C.c_float)]


class TextCfg(C.Structure):
    _fields_ = [("format", C.c_int32), ("flags", C.c_int32), ("first_global_id", C.c_int64)]


class TextStats(C.Structure):
    _fields_ = [("nreads", C.c_int64), ("bases", C.c_int64), ("packed_bytes", C.c_int64), ("chunk_bytes", C.c_int64), ("lines", C.c_int64),
                ("format", C.c_int32), ("reserved", C.c_int32), ("ms_total", C.c_float), ("ms_index", C.c_float), ("ms_encode", C.c_float)]


TEXT_FORMATS = {"auto": 0, "fasta": 1, "fastq": 2}      # ELBA_TEXT_AUTO / _FASTA / _FASTQ


class AlignStats(C.Structure):
    _fields_ = [("nalignments", C.c_int64), ("seeds_rejected", C.c_int64), ("passed", C.c_int64), ("contained", C.c_int64),
                ("extensions_strided", C.c_int64), ("cells", C.c_int64), ("ms_total", C.c_float), ("ms_extend", C.c_float)]


class StringStats(C.Structure):
    _fields_ = [("nreads", C.c_int64), ("nedges", C.c_int64), ("bad_reads", C.c_int64), ("edges_passed", C.c_int64), ("contained_reads", C.c_int64),
                ("edges_kept", C.c_int64), ("products", C.c_int64), ("marked", C.c_int64), ("removed", C.c_int64), ("nnz", C.c_int64),
                ("iterations", C.c_int32), ("reserved", C.c_int32), ("ms_total", C.c_float), ("ms_minplus", C.c_float)]


class ContigStats(C.Structure):
    _fields_ = [("nreads", C.c_int64), ("branches", C.c_int64), ("components", C.c_int64), ("used_components", C.c_int64), ("contigs", C.c_int64),
                ("cycles", C.c_int64), ("contig_reads", C.c_int64), ("bases", C.c_int64), ("longest", C.c_int64), ("ms_total", C.c_float), ("ms_rank", C.c_float)]


class ContigCfg(C.Structure):
    _fields_ = [("flags", C.c_int32), ("reserved", C.c_int32 * 3)]


CONTIG_CIRCULAR, CONTIG_SINGLETONS = 1, 2          # elba_contig_cfg.flags
CONTIG_KIND_PATH, CONTIG_KIND_CIRCULAR, CONTIG_KIND_SINGLE = 0, 1, 2


class Contigs(C.Structure):
    _fields_ = [("n", C.c_int64), ("seq_off", C.c_void_p), ("seq", C.c_void_p), ("chain_off", C.c_void_p), ("chain_read", C.c_void_p),
                ("chain_prefix", C.c_void_p), ("chain_strand", C.c_void_p)]


class Links(C.Structure):
    _fields_ = [("n", C.c_int64), ("links", C.c_void_p)]


class GraphStats(C.Structure):
    _fields_ = [("segments", C.c_int64), ("candidates", C.c_int64), ("links", C.c_int64), ("closures", C.c_int64), ("twisted", C.c_int64),
                ("unplaced", C.c_int64), ("clamped", C.c_int64), ("asymmetric", C.c_int64), ("ms_total", C.c_float), ("reserved", C.c_int32)]


# elba_link_t: 24 bytes
LINK_DTYPE = np.dtype([("from", "<u4"), ("to", "<u4"), ("from_read", "<u4"), ("to_read", "<u4"), ("overlap", "<i4"), ("from_rev", "u1"), ("to_rev", "u1"),
                       ("flags", "u1"), ("reserved", "u1")])
LINK_CLOSURE = 1          # elba_link_t.flags bit 0


CC_STRING, CC_OVERLAPS = 0, 1          # elba_cc_cfg.graph
CC_BASES = 1                           # elba_cc_cfg.flags
_CC_GRAPHS = {"string": CC_STRING, "overlaps": CC_OVERLAPS}
_CC_WEIGHTS = {"reads": 0, "bases": 1}


class CcCfg(C.Structure):
    _fields_ = [("graph", C.c_int32), ("flags", C.c_int32), ("reserved", C.c_int32 * 2)]


class Components(C.Structure):
    _fields_ = [("nreads", C.c_int64), ("n", C.c_int64), ("comp_of_read", C.c_void_p), ("first_read", C.c_void_p), ("reads", C.c_void_p), ("bases", C.c_void_p),
                ("edges", C.c_void_p), ("branches", C.c_void_p), ("ends", C.c_void_p)]


class CcStats(C.Structure):
    _fields_ = [("nreads", C.c_int64), ("edges", C.c_int64), ("components", C.c_int64), ("used_components", C.c_int64), ("isolated", C.c_int64),
                ("largest_reads", C.c_int64), ("largest_bases", C.c_int64), ("passes", C.c_int32), ("reserved", C.c_int32), ("ms_total", C.c_float), ("ms_label", C.c_float)]


class PartCfg(C.Structure):
    _fields_ = [("graph", C.c_int32), ("nparts", C.c_int32), ("weight", C.c_int32), ("min_reads", C.c_int32), ("reserved", C.c_int32 * 4)]


INDUCE_BASES, INDUCE_HOST = 1, 2       # elba_induce_cfg.flags


class InduceCfg(C.Structure):
    _fields_ = [("part", C.c_int32), ("flags", C.c_int32), ("reserved", C.c_int32 * 2)]


class Induced(C.Structure):
    _fields_ = [("reads", C.c_int64), ("pairs", C.c_int64), ("packed_bytes", C.c_int64)] + \
               [(n, C.c_void_p) for n in ("d_old_of_new", "d_packed", "d_byte_off", "d_len", "d_rows", "d_cols", "d_vals", "d_outside_aligned", "d_outside_passed")] + \
               [(n, C.c_void_p) for n in ("old_of_new", "packed", "byte_off", "len", "rows", "cols", "vals", "outside_aligned", "outside_passed")]


class InduceStats(C.Structure):
    _fields_ = [(n, C.c_int64) for n in ("nreads_in", "pairs_in", "reads", "pairs", "bases", "packed_bytes", "split_pairs", "split_passed", "id_base")] + \
               [("ms_total", C.c_float), ("ms_pairs", C.c_float), ("ms_gather", C.c_float)]


class PlaceCfg(C.Structure):
    _fields_ = [("skip_flags", C.c_int32), ("reserved", C.c_int32 * 3)]


class Placements(C.Structure):
    _fields_ = [("nreads", C.c_int64), ("ncontigs", C.c_int64), ("reads", C.c_void_p), ("seg_off", C.c_void_p), ("seg_start", C.c_void_p), ("seg_depth", C.c_void_p),
                ("credited_reads", C.c_void_p), ("credited_bases", C.c_void_p)]


class PlaceStats(C.Structure):
    _fields_ = [("nreads", C.c_int64), ("chain", C.c_int64), ("anchored", C.c_int64), ("unanchored", C.c_int64), ("skipped", C.c_int64), ("empty", C.c_int64),
                ("candidates", C.c_int64), ("clipped", C.c_int64), ("outside", C.c_int64), ("wrapped", C.c_int64), ("segments", C.c_int64), ("max_depth", C.c_int64),
                ("credited_bases", C.c_int64), ("ms_total", C.c_float), ("reserved", C.c_int32)]


# elba_placement_t: 24 bytes
PLACEMENT_DTYPE = np.dtype([("start", "<i8"), ("contig", "<i4"), ("anchor", "<u4"), ("score", "<i4"), ("strand", "u1"), ("kind", "u1"), ("flags", "u1"), ("reserved", "u1")])
PLACE_NONE, PLACE_CHAIN, PLACE_ANCHORED = 0, 1, 2      # elba_placement_t.kind
PLACE_CLIPPED, PLACE_OUTSIDE, PLACE_WRAPPED = 1, 2, 4  # elba_placement_t.flags


class PolishCfg(C.Structure):
    _fields_ = [("skip_flags", C.c_int32), ("band", C.c_int32), ("max_diff_q16", C.c_int32), ("min_depth", C.c_int32), ("flags", C.c_int32), ("reserved", C.c_int32 * 3)]


class Polished(C.Structure):
    _fields_ = [("n", C.c_int64), ("seq_off", C.c_void_p), ("seq", C.c_void_p), ("voters", C.c_void_p), ("substituted", C.c_void_p), ("deleted", C.c_void_p),
                ("inserted", C.c_void_p), ("nreads", C.c_int64), ("col_off", C.c_void_p), ("col", C.c_void_p), ("gap", C.c_void_p), ("reads", C.c_void_p)]


class PolishStats(C.Structure):
    _fields_ = [("nreads", C.c_int64), ("voted", C.c_int64), ("rejected", C.c_int64), ("outside", C.c_int64), ("low_depth_columns", C.c_int64), ("bases_before", C.c_int64),
                ("bases_after", C.c_int64), ("sum_dist", C.c_int64), ("cells", C.c_int64), ("batches", C.c_int64), ("ms_total", C.c_float), ("ms_align", C.c_float)]


# elba_polish_read_t: 16 bytes
POLISH_READ_DTYPE = np.dtype([("dist", "<i4"), ("n", "<i4"), ("end_j", "<i4"), ("status", "<i4")])
POLISH_EXPORT_VOTES = 1                                                          # elba_polish_cfg.flags
POLISH_NOT_PLACED, POLISH_OUTSIDE, POLISH_REJECTED, POLISH_VOTED = 0, 1, 2, 3    # elba_polish_read_t.status


class PileupCfg(C.Structure):
    _fields_ = [("mode", C.c_int32), ("margin", C.c_int32), ("min_depth", C.c_int32), ("min_run", C.c_int32), ("trim_len", C.c_int32), ("reserved", C.c_int32)]


class PileupStats(C.Structure):
    _fields_ = [("nreads", C.c_int64), ("pairs", C.c_int64), ("intervals", C.c_int64), ("segments", C.c_int64), ("max_depth", C.c_int64),
                ("unsupported", C.c_int64), ("split", C.c_int64), ("trimmed", C.c_int64), ("trimmed_bases", C.c_int64), ("ms_total", C.c_float), ("reserved", C.c_float)]


class Pileup(C.Structure):
    _fields_ = [("n", C.c_int64), ("nseg", C.c_int64), ("seg_off", C.c_void_p), ("seg_start", C.c_void_p), ("seg_depth", C.c_void_p),
                ("trim_beg", C.c_void_p), ("trim_end", C.c_void_p), ("flags", C.c_void_p)]


class TrimCfg(C.Structure):
    _fields_ = [("mode", C.c_int32), ("min_len", C.c_int32), ("reserved", C.c_int32 * 2)]


class TrimStats(C.Structure):
    _fields_ = [("nreads_in", C.c_int64), ("pieces", C.c_int64), ("reads_dropped", C.c_int64), ("reads_split", C.c_int64), ("reads_unchanged", C.c_int64),
                ("bases_in", C.c_int64), ("bases_out", C.c_int64), ("packed_bytes", C.c_int64), ("longest", C.c_int64), ("ms_total", C.c_float), ("ms_repack", C.c_float)]


class TrimMap(C.Structure):
    _fields_ = [("n", C.c_int64), ("src_read", C.c_void_p), ("src_beg", C.c_void_p), ("src_end", C.c_void_p)]


class TipCfg(C.Structure):
    _fields_ = [("max_tip_reads", C.c_int32), ("rounds", C.c_int32), ("reserved", C.c_int32 * 2)]


class TipStats(C.Structure):
    _fields_ = [("nreads", C.c_int64), ("nnz_before", C.c_int64), ("nnz_after", C.c_int64), ("dead_ends", C.c_int64), ("tips", C.c_int64),
                ("reads_removed", C.c_int64), ("entries_removed", C.c_int64), ("spared_anchors", C.c_int64), ("rounds_run", C.c_int32), ("reserved", C.c_int32),
                ("ms_total", C.c_float), ("ms_compact", C.c_float)]


class BubbleCfg(C.Structure):
    _fields_ = [("max_arm_reads", C.c_int32), ("rounds", C.c_int32), ("reserved", C.c_int32 * 2)]


class BubbleStats(C.Structure):
    _fields_ = [("nreads", C.c_int64), ("nnz_before", C.c_int64), ("nnz_after", C.c_int64), ("anchors", C.c_int64), ("arms", C.c_int64), ("bubbles", C.c_int64),
                ("arms_removed", C.c_int64), ("reads_removed", C.c_int64), ("entries_removed", C.c_int64), ("rounds_run", C.c_int32), ("reserved", C.c_int32),
                ("ms_total", C.c_float), ("ms_compact", C.c_float)]


class WeakCfg(C.Structure):
    _fields_ = [("min_ratio_q16", C.c_int32), ("reserved", C.c_int32 * 3)]


class WeakStats(C.Structure):
    _fields_ = [("nreads", C.c_int64), ("nnz_before", C.c_int64), ("nnz_after", C.c_int64), ("branch_sides", C.c_int64), ("weak_entries", C.c_int64),
                ("entries_removed", C.c_int64), ("sides_emptied", C.c_int64), ("ms_total", C.c_float), ("ms_compact", C.c_float)]


class BridgeCfg(C.Structure):
    _fields_ = [("max_bridge_reads", C.c_int32), ("min_flank_reads", C.c_int32), ("reserved", C.c_int32 * 2)]


class BridgeStats(C.Structure):
    _fields_ = [("nreads", C.c_int64), ("nnz_before", C.c_int64), ("nnz_after", C.c_int64), ("anchors", C.c_int64), ("chains", C.c_int64),
                ("long_flanks", C.c_int64), ("bridges", C.c_int64), ("reads_removed", C.c_int64), ("entries_removed", C.c_int64),
                ("ms_total", C.c_float), ("ms_compact", C.c_float)]


class StarCfg(C.Structure):
    _fields_ = [("rounds", C.c_int32), ("reserved", C.c_int32 * 3)]


class StarStats(C.Structure):
    _fields_ = [("nreads", C.c_int64), ("nnz_before", C.c_int64), ("nnz_after", C.c_int64), ("centres", C.c_int64), ("pairs0", C.c_int64),
                ("pairs1", C.c_int64), ("pairs2", C.c_int64), ("pairs3", C.c_int64), ("reads_removed", C.c_int64), ("entries_removed", C.c_int64),
                ("rounds_run", C.c_int32), ("reserved", C.c_int32), ("ms_total", C.c_float), ("ms_compact", C.c_float)]


class Overlaps(C.Structure):
    _fields_ = [("n", C.c_int64), ("rows", C.c_void_p), ("cols", C.c_void_p), ("vals", C.c_void_p)]


# elba_overlap_t (include/elba_amd.h): the fields Overlap::extend_overlap fills (src/Overlap.cpp:24-73)
OVERLAP_DTYPE = np.dtype([("begQ", "<i4"), ("begT", "<i4"), ("endQ", "<i4"), ("endT", "<i4"), ("score", "<i4"), ("suffix", "<i4"), ("suffixT", "<i4"),
                          ("direction", "i1"), ("directionT", "i1"), ("rc", "u1"), ("passed", "u1"), ("containedQ", "u1"), ("containedT", "u1"), ("kind", "u1"), ("reserved", "u1")])


class Dcsc(C.Structure):
    _fields_ = [("nrows", C.c_int64), ("ncols", C.c_int64), ("nnz", C.c_int64), ("nzc", C.c_int64),
                ("jc", C.c_void_p), ("cp", C.c_void_p), ("ir", C.c_void_p), ("numx", C.c_void_p)]


class Csr(C.Structure):
    _fields_ = [("nrows", C.c_int64), ("ncols", C.c_int64), ("nnz", C.c_int64), ("rowptr", C.c_void_p), ("col", C.c_void_p), ("val", C.c_void_p)]


class KmerMatrix(C.Structure):
    _fields_ = [("nrows", C.c_int64), ("ncols", C.c_int64), ("nnz", C.c_int64), ("kmers", C.c_void_p), ("kmers_lo", C.c_void_p), ("kmers_lo2", C.c_void_p), ("colptr", C.c_void_p),
                ("csc_row", C.c_void_p), ("csc_val", C.c_void_p), ("rowptr", C.c_void_p), ("csr_col", C.c_void_p), ("csr_val", C.c_void_p)]


class DeviceView(C.Structure):
    _fields_ = [("M", C.c_int64), ("N", C.c_int64), ("Z", C.c_int64), ("Y", C.c_int64),
                ("a_rowptr", C.c_void_p), ("a_csr", C.c_void_p), ("a_colptr", C.c_void_p), ("a_csc", C.c_void_p),
                ("b_rowptr", C.c_void_p), ("b_col", C.c_void_p), ("b_val", C.c_void_p), ("stream", C.c_void_p),
                ("a_csr_format", C.c_uint32), ("a_csr_pos_mask", C.c_uint32), ("a_kmers", C.c_void_p),
                ("a_gather_slots", C.c_int64), ("a_slot_kid", C.c_void_p)]


class SynthCfg(C.Structure):
    _fields_ = [("seed", C.c_uint64), ("genome_length", C.c_int64), ("depth", C.c_double), ("avg_len", C.c_double), ("sd_len", C.c_double),
                ("min_len", C.c_int64), ("error_rate", C.c_double), ("repeat_families", C.c_int32), ("repeat_fraction", C.c_double),
                ("repeat_len", C.c_int64), ("first_read", C.c_int64), ("num_reads", C.c_int64)]


class SynthReads(C.Structure):
    _fields_ = [("nreads", C.c_int64), ("total_reads", C.c_int64), ("packed_bytes", C.c_int64), ("total_bases", C.c_int64),
                ("packed", C.c_void_p), ("byte_off", C.c_void_p), ("len", C.c_void_p), ("genome_pos", C.c_void_p), ("strand", C.c_void_p)]


EXPORTED_SYMBOLS = [
    "elba_abi_version", "elba_strerror", "elba_last_error", "elba_ctx_create", "elba_ctx_destroy", "elba_set_reads", "elba_set_reads_device",
    "elba_count_kmers", "elba_create_kmer_matrix", "elba_set_kmer_matrix", "elba_create_seed_matrix", "elba_export_dcsc", "elba_free_dcsc",
    "elba_export_csr", "elba_free_csr", "elba_export_kmer_matrix", "elba_free_kmer_matrix", "elba_kmer_histogram", "elba_get_device_view", "elba_set_option",
    "elba_align_seeds", "elba_export_overlaps", "elba_free_overlaps", "elba_set_overlaps", "elba_transitive_reduction", "elba_export_string_graph", "elba_export_read_flags", "elba_set_reads_fasta", "elba_export_reads", "elba_dist_set_all_reads",
    "elba_synth_num_reads", "elba_synth_generate", "elba_synth_free",
    "elba_kmer_hash_owner", "elba_dist_value_histogram", "elba_dist_set_owner_ranges", "elba_dist_set_kmer_id_base", "elba_dist_count_owners", "elba_dist_fill_send", "elba_dist_packed_format", "elba_dist_fill_send_packed", "elba_dist_unpack_records", "elba_dist_count_records", "elba_dist_get_reliable_kmers", "elba_dist_copy_reliable_kmers",
    "elba_dist_set_global_kmers", "elba_dist_panel_counts", "elba_dist_panel_fill", "elba_dist_panel_counts_win", "elba_dist_panel_fill_win", "elba_dist_set_panel",
    "elba_seed_matrix_begin", "elba_seed_matrix_fill", "elba_seed_matrix_end", "elba_set_stream", "elba_seed_matrix_send", "elba_seed_matrix_recv", "elba_set_kmer_matrix_device", "elba_export_triples_device", "elba_get_stat", "elba_release_workspace",
    "elba_generate_contigs", "elba_export_contigs", "elba_free_contigs", "elba_export_read_contigs", "elba_generate_contigs_ex", "elba_export_contig_kinds",
    "elba_read_pileup", "elba_export_pileup", "elba_free_pileup", "elba_prune_reads",
    "elba_trim_reads", "elba_export_trim_map", "elba_free_trim_map", "elba_get_trimmed_reads_device", "elba_adopt_trimmed_reads",
    "elba_clip_tips", "elba_pop_bubbles", "elba_cut_weak_overlaps", "elba_cut_bridges", "elba_resolve_stars",
    "elba_set_reads_text", "elba_export_read_index",
    "elba_export_assembly_links", "elba_free_links",
    "elba_place_reads", "elba_free_placements",
    "elba_polish_contigs", "elba_free_polished",
    "elba_graph_components", "elba_free_components", "elba_partition_components",
    "elba_induce_part", "elba_free_induced", "elba_set_overlaps_device", "elba_set_outside_counts", "elba_set_outside_counts_device",
]

_lib = None


def load_library():
    """Loads libelba_amd.so or raises: the product path never falls back to anything else."""
    global _lib
    if _lib is not None:
        return _lib
    p = lib_path()
    # One HIP runtime per process: PyTorch bundles its own libamdhip64 (same SONAME as the system one).  Whichever is loaded first
    # serves both; when the system one came first, torch found no GPU afterwards (measured on the GPU box: "No HIP GPUs are available").
    # The binding hands device memory to torch tensors (tests, bench.py, the multi-GPU driver), so torch's copy is loaded first when there is one.
    try:
        import importlib.util
        spec = importlib.util.find_spec("torch")
        if spec is not None and spec.submodule_search_locations:
            hip = os.path.join(list(spec.submodule_search_locations)[0], "lib", "libamdhip64.so")
            if os.path.exists(hip):
                C.CDLL(hip, mode=C.RTLD_GLOBAL)
    except Exception:      # noqa: BLE001 — without torch the system runtime is the only one
        pass
    if not os.path.exists(p):
        raise ElbaError(-1, "libelba_amd.so is not built (%s); run `python -c 'import __graft_entry__ as g; g.build()'` or `make -C elba_amd/csrc`" % p)
    L = C.CDLL(p)
    vp, i64, i32 = C.c_void_p, C.c_int64, C.c_int
    L.elba_abi_version.restype = i32
    L.elba_strerror.restype = C.c_char_p; L.elba_strerror.argtypes = [i32]
    L.elba_last_error.restype = C.c_char_p; L.elba_last_error.argtypes = [vp]
    L.elba_ctx_create.restype = i32; L.elba_ctx_create.argtypes = [C.POINTER(vp), C.POINTER(Cfg)]
    L.elba_ctx_destroy.restype = None; L.elba_ctx_destroy.argtypes = [vp]
    L.elba_set_reads.restype = i32; L.elba_set_reads.argtypes = [vp, vp, vp, vp, i64, i64]
    L.elba_set_reads_device.restype = i32; L.elba_set_reads_device.argtypes = [vp, vp, i64, vp, vp, i64, i64]
    L.elba_set_reads_fasta.restype = i32; L.elba_set_reads_fasta.argtypes = [vp, vp, i64, C.c_uint64, vp, i64, i64, C.POINTER(IngestStats)]
    L.elba_export_reads.restype = i32; L.elba_export_reads.argtypes = [vp, vp, i64, vp, vp, i64]
    L.elba_set_reads_text.restype = i32; L.elba_set_reads_text.argtypes = [vp, vp, i64, C.c_uint64, C.POINTER(TextCfg), C.POINTER(TextStats)]
    L.elba_export_read_index.restype = i32; L.elba_export_read_index.argtypes = [vp, vp, vp, vp, i64]
    L.elba_count_kmers.restype = i32; L.elba_count_kmers.argtypes = [vp, C.POINTER(KmerStats)]
    L.elba_create_kmer_matrix.restype = i32; L.elba_create_kmer_matrix.argtypes = [vp, C.POINTER(MatrixStats)]
    L.elba_set_kmer_matrix.restype = i32; L.elba_set_kmer_matrix.argtypes = [vp, i64, i64, i64, vp, vp, vp, C.POINTER(MatrixStats)]
    L.elba_set_kmer_matrix_device.restype = i32; L.elba_set_kmer_matrix_device.argtypes = [vp, i64, i64, i64, vp, vp, vp, C.POINTER(MatrixStats)]
    L.elba_export_triples_device.restype = i32; L.elba_export_triples_device.argtypes = [vp, vp, vp, vp]
    L.elba_create_seed_matrix.restype = i32; L.elba_create_seed_matrix.argtypes = [vp, C.POINTER(OverlapStats)]
    L.elba_align_seeds.restype = i32; L.elba_align_seeds.argtypes = [vp, i32, i32, i32, i32, C.POINTER(AlignStats)]
    L.elba_export_overlaps.restype = i32; L.elba_export_overlaps.argtypes = [vp, C.POINTER(Overlaps)]
    L.elba_free_overlaps.restype = None; L.elba_free_overlaps.argtypes = [C.POINTER(Overlaps)]
    L.elba_set_overlaps.restype = i32; L.elba_set_overlaps.argtypes = [vp, i64, vp, vp, vp, i64]
    L.elba_transitive_reduction.restype = i32; L.elba_transitive_reduction.argtypes = [vp, C.c_double, i32, C.POINTER(StringStats)]
    L.elba_export_string_graph.restype = i32; L.elba_export_string_graph.argtypes = [vp, C.POINTER(Overlaps)]
    L.elba_export_read_flags.restype = i32; L.elba_export_read_flags.argtypes = [vp, vp, i64]
    L.elba_clip_tips.restype = i32; L.elba_clip_tips.argtypes = [vp, C.POINTER(TipCfg), C.POINTER(TipStats)]
    L.elba_pop_bubbles.restype = i32; L.elba_pop_bubbles.argtypes = [vp, C.POINTER(BubbleCfg), C.POINTER(BubbleStats)]
    L.elba_cut_weak_overlaps.restype = i32; L.elba_cut_weak_overlaps.argtypes = [vp, C.POINTER(WeakCfg), C.POINTER(WeakStats)]
    L.elba_cut_bridges.restype = i32; L.elba_cut_bridges.argtypes = [vp, C.POINTER(BridgeCfg), C.POINTER(BridgeStats)]
    L.elba_resolve_stars.restype = i32; L.elba_resolve_stars.argtypes = [vp, C.POINTER(StarCfg), C.POINTER(StarStats)]
    L.elba_generate_contigs.restype = i32; L.elba_generate_contigs.argtypes = [vp, C.POINTER(ContigStats)]
    L.elba_generate_contigs_ex.restype = i32; L.elba_generate_contigs_ex.argtypes = [vp, C.POINTER(ContigCfg), C.POINTER(ContigStats)]
    L.elba_export_contig_kinds.restype = i32; L.elba_export_contig_kinds.argtypes = [vp, vp, i64]
    L.elba_export_contigs.restype = i32; L.elba_export_contigs.argtypes = [vp, C.POINTER(Contigs)]
    L.elba_free_contigs.restype = None; L.elba_free_contigs.argtypes = [C.POINTER(Contigs)]
    L.elba_export_read_contigs.restype = i32; L.elba_export_read_contigs.argtypes = [vp, vp, i64]
    L.elba_export_assembly_links.restype = i32; L.elba_export_assembly_links.argtypes = [vp, C.POINTER(Links), C.POINTER(GraphStats)]
    L.elba_free_links.restype = None; L.elba_free_links.argtypes = [C.POINTER(Links)]
    L.elba_place_reads.restype = i32; L.elba_place_reads.argtypes = [vp, C.POINTER(PlaceCfg), C.POINTER(Placements), C.POINTER(PlaceStats)]
    L.elba_free_placements.restype = None; L.elba_free_placements.argtypes = [C.POINTER(Placements)]
    L.elba_polish_contigs.restype = i32; L.elba_polish_contigs.argtypes = [vp, C.POINTER(PolishCfg), C.POINTER(Polished), C.POINTER(PolishStats)]
    L.elba_free_polished.restype = None; L.elba_free_polished.argtypes = [C.POINTER(Polished)]
    L.elba_graph_components.restype = i32; L.elba_graph_components.argtypes = [vp, C.POINTER(CcCfg), C.POINTER(Components), C.POINTER(CcStats)]
    L.elba_free_components.restype = None; L.elba_free_components.argtypes = [C.POINTER(Components)]
    L.elba_partition_components.restype = i32; L.elba_partition_components.argtypes = [vp, C.POINTER(PartCfg), vp, i64, vp]
    L.elba_induce_part.restype = i32; L.elba_induce_part.argtypes = [vp, C.POINTER(InduceCfg), vp, i64, C.POINTER(Induced), C.POINTER(InduceStats)]
    L.elba_free_induced.restype = None; L.elba_free_induced.argtypes = [C.POINTER(Induced)]
    L.elba_set_overlaps_device.restype = i32; L.elba_set_overlaps_device.argtypes = [vp, i64, vp, vp, vp, i64]
    L.elba_set_outside_counts.restype = i32; L.elba_set_outside_counts.argtypes = [vp, i64, vp, vp]
    L.elba_set_outside_counts_device.restype = i32; L.elba_set_outside_counts_device.argtypes = [vp, i64, vp, vp]
    L.elba_read_pileup.restype = i32; L.elba_read_pileup.argtypes = [vp, C.POINTER(PileupCfg), C.POINTER(PileupStats)]
    L.elba_export_pileup.restype = i32; L.elba_export_pileup.argtypes = [vp, C.POINTER(Pileup)]
    L.elba_free_pileup.restype = None; L.elba_free_pileup.argtypes = [C.POINTER(Pileup)]
    L.elba_prune_reads.restype = i32; L.elba_prune_reads.argtypes = [vp, i32, C.POINTER(C.c_int64)]
    L.elba_trim_reads.restype = i32; L.elba_trim_reads.argtypes = [vp, C.POINTER(TrimCfg), C.POINTER(TrimStats)]
    L.elba_export_trim_map.restype = i32; L.elba_export_trim_map.argtypes = [vp, C.POINTER(TrimMap)]
    L.elba_free_trim_map.restype = None; L.elba_free_trim_map.argtypes = [C.POINTER(TrimMap)]
    L.elba_get_trimmed_reads_device.restype = i32; L.elba_get_trimmed_reads_device.argtypes = [vp, C.POINTER(vp), C.POINTER(i64), C.POINTER(vp), C.POINTER(vp), C.POINTER(i64)]
    L.elba_adopt_trimmed_reads.restype = i32; L.elba_adopt_trimmed_reads.argtypes = [vp]
    L.elba_export_dcsc.restype = i32; L.elba_export_dcsc.argtypes = [vp, i64, i64, i64, i64, C.POINTER(Dcsc)]
    L.elba_free_dcsc.restype = None; L.elba_free_dcsc.argtypes = [C.POINTER(Dcsc)]
    L.elba_export_csr.restype = i32; L.elba_export_csr.argtypes = [vp, i64, i64, C.POINTER(Csr)]
    L.elba_free_csr.restype = None; L.elba_free_csr.argtypes = [C.POINTER(Csr)]
    L.elba_export_kmer_matrix.restype = i32; L.elba_export_kmer_matrix.argtypes = [vp, C.POINTER(KmerMatrix)]
    L.elba_free_kmer_matrix.restype = None; L.elba_free_kmer_matrix.argtypes = [C.POINTER(KmerMatrix)]
    L.elba_kmer_histogram.restype = i32; L.elba_kmer_histogram.argtypes = [vp, vp, i64]
    L.elba_get_device_view.restype = i32; L.elba_get_device_view.argtypes = [vp, C.POINTER(DeviceView)]
    L.elba_set_option.restype = i32; L.elba_set_option.argtypes = [vp, C.c_char_p, i64]
    L.elba_get_stat.restype = i32; L.elba_get_stat.argtypes = [vp, C.c_char_p, C.POINTER(C.c_int64)]
    L.elba_release_workspace.restype = i32; L.elba_release_workspace.argtypes = [vp]
    L.elba_kmer_hash_owner.restype = i32; L.elba_kmer_hash_owner.argtypes = [vp, vp, i64, i32, vp, vp]
    L.elba_synth_num_reads.restype = i64; L.elba_synth_num_reads.argtypes = [C.POINTER(SynthCfg)]
    L.elba_synth_generate.restype = i32; L.elba_synth_generate.argtypes = [C.POINTER(SynthCfg), C.POINTER(SynthReads)]
    L.elba_synth_free.restype = None; L.elba_synth_free.argtypes = [C.POINTER(SynthReads)]
    _lib = L
    return L


def _copy(ptr, n, dtype):
    dt = np.dtype(dtype)
    if n == 0 or not ptr:
        return np.zeros(0, dtype=dt)
    buf = (C.c_char * (n * dt.itemsize)).from_address(ptr)
    return np.frombuffer(buf, dtype=dt, count=n).copy()


def _copy_from_device(dev_ptr, n, dtype):
    """n items of dtype from a device address of the library into a fresh numpy array: hipMemcpy of the HIP runtime the library itself
    is linked to (looked up through the library's handle, so no second runtime enters the process)."""
    out = np.empty(int(n), dtype=dtype)
    if n:
        f = load_library().hipMemcpy
        f.restype = C.c_int; f.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        rc = f(out.ctypes.data, int(dev_ptr), out.nbytes, 2)      # hipMemcpyDeviceToHost
        if rc:
            raise ElbaError(ELBA_ERR_HIP, "hipMemcpy device to host failed: %d" % rc)
    return out


def _stats(s):
    return {f[0]: getattr(s, f[0]) for f in s._fields_}


def synth_reads(seed, genome_length, depth, avg_len, sd_len, error_rate=0.0, min_len=100, repeat_families=0, repeat_fraction=0.0,
                repeat_len=0, first_read=0, num_reads=-1):
    """Generates (packed u8, byte_off u64, len u32, info) with the native generator (host code; no GPU needed)."""
    L = load_library()
    cfg = SynthCfg(seed, genome_length, depth, avg_len, sd_len, min_len, error_rate, repeat_families, repeat_fraction, repeat_len, first_read, num_reads)
    out = SynthReads()
    rc = L.elba_synth_generate(C.byref(cfg), C.byref(out))
    if rc:
        raise ElbaError(rc, "elba_synth_generate failed")
    try:
        packed = _copy(out.packed, out.packed_bytes + 16, np.uint8)
        off = _copy(out.byte_off, out.nreads, np.uint64)
        ln = _copy(out.len, out.nreads, np.uint32)
        info = dict(nreads=out.nreads, total_reads=out.total_reads, total_bases=out.total_bases,
                    genome_pos=_copy(out.genome_pos, out.nreads, np.int64), strand=_copy(out.strand, out.nreads, np.uint8))
    finally:
        L.elba_synth_free(C.byref(out))
    return packed, off, ln, info


class Engine:
    """One context on one GPU.  Method names follow the reference's free functions (include/KmerOps.hpp:24-31,
    include/SharedSeeds.hpp:98-99); each is a single C-ABI call."""

    def __init__(self, k, lower, upper, device=0, workspace_hint_bytes=0, flags=0, timing_stride=0, options=None):
        self.L = load_library()
        self.h = C.c_void_p()
        cfg = Cfg(k, lower, upper, device, workspace_hint_bytes, flags, timing_stride)
        rc = self.L.elba_ctx_create(C.byref(self.h), C.byref(cfg))
        if rc:
            self.h = C.c_void_p()
            raise ElbaError(rc, self.L.elba_strerror(rc).decode())
        self.k, self.lower, self.upper, self.device = k, lower, upper, device
        for name, value in (options or {}).items():
            self.set_option(name, value)

    def close(self):
        if getattr(self, "h", None) and self.h.value:
            self.L.elba_ctx_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc):
        if rc:
            raise ElbaError(rc, "%s: %s" % (self.L.elba_strerror(rc).decode(), self.L.elba_last_error(self.h).decode()))

    # --- inputs ---
    def set_reads(self, packed, byte_off, lens, first_global_id=0):
        packed = np.ascontiguousarray(packed, dtype=np.uint8)
        byte_off = np.ascontiguousarray(byte_off, dtype=np.uint64)
        lens = np.ascontiguousarray(lens, dtype=np.uint32)
        self._check(self.L.elba_set_reads(self.h, packed.ctypes.data, byte_off.ctypes.data, lens.ctypes.data, len(lens), first_global_id))

    def set_reads_device(self, d_packed, packed_bytes, d_byte_off, d_len, nreads, first_global_id=0):
        self._check(self.L.elba_set_reads_device(self.h, d_packed, packed_bytes, d_byte_off, d_len, nreads, first_global_id))

    def set_reads_fasta(self, chunk, chunk_file_offset, recs, first_global_id=0):
        """FastaIndex::getmydna (src/FastaIndex.cpp:191-290) with the 2-bit encoding on the GPU: `chunk` = raw FASTA bytes from
        `chunk_file_offset` on, `recs` = this rank's .fai records (elba_amd.fasta.FAI_DTYPE)."""
        buf = np.frombuffer(chunk, dtype=np.uint8) if not isinstance(chunk, np.ndarray) else np.ascontiguousarray(chunk, dtype=np.uint8)
        recs = np.ascontiguousarray(recs)
        assert recs.dtype.itemsize == 24
        st = IngestStats()
        self._check(self.L.elba_set_reads_fasta(self.h, buf.ctypes.data if buf.size else None, buf.size, chunk_file_offset, recs.ctypes.data if recs.size else None,
                                                len(recs), first_global_id, C.byref(st)))
        return _stats(st)

    def set_reads_text(self, chunk, chunk_file_offset=0, fmt="auto", first_global_id=0):
        """Reads from raw FASTA or FASTQ text without a .fai (elba_set_reads_text): `chunk` = the file's bytes from `chunk_file_offset` on,
        beginning at a record; the index is built and the reads are 2-bit encoded on the GPU.  fmt: "auto" (by the first byte), "fasta",
        "fastq".  Returns the stats as a dict.  The binding keeps a reference to the chunk: export_read_index slices the names from it."""
        buf = np.frombuffer(chunk, dtype=np.uint8) if not isinstance(chunk, np.ndarray) else np.ascontiguousarray(chunk, dtype=np.uint8)
        cfg = TextCfg(TEXT_FORMATS[fmt], 0, first_global_id)
        st = TextStats()
        self._check(self.L.elba_set_reads_text(self.h, buf.ctypes.data if buf.size else None, buf.size, chunk_file_offset, C.byref(cfg), C.byref(st)))
        self._text_chunk, self._text_chunk_offset, self._text_nreads = buf, int(chunk_file_offset), int(st.nreads)
        return _stats(st)

    def export_read_index(self):
        """(names, recs) of the reads that came in through set_reads_text, in the shape fasta.read_fai returns: the records
        (fasta.FAI_DTYPE, file offsets) from the library, the names sliced on the host from the chunk of that call."""
        from .fasta import FAI_DTYPE
        m = getattr(self, "_text_nreads", 0)      # (a stale count cannot pass: the library checks the state first)
        recs = np.zeros(m, dtype=FAI_DTYPE); npos = np.zeros(m, dtype=np.uint64); nlen = np.zeros(m, dtype=np.uint32)
        self._check(self.L.elba_export_read_index(self.h, recs.ctypes.data, npos.ctypes.data, nlen.ctypes.data, m))
        raw = self._text_chunk.tobytes()
        lo = npos.astype(np.int64) - self._text_chunk_offset
        names = [raw[a:a + l].decode() for a, l in zip(lo.tolist(), nlen.tolist())]
        return names, recs

    def export_read_index_raw(self):
        """(recs, name_pos, name_len) as the library keeps them (elba_export_read_index)."""
        from .fasta import FAI_DTYPE
        m = getattr(self, "_text_nreads", 0)      # (a stale count cannot pass: the library checks the state first)
        recs = np.zeros(m, dtype=FAI_DTYPE); npos = np.zeros(m, dtype=np.uint64); nlen = np.zeros(m, dtype=np.uint32)
        self._check(self.L.elba_export_read_index(self.h, recs.ctypes.data, npos.ctypes.data, nlen.ctypes.data, m))
        return recs, npos, nlen

    def set_reads_file(self, path, fmt="auto", first_global_id=0):
        """A whole FASTA or FASTQ file through set_reads_text.  A name that ends in .gz is inflated with Python's gzip on the host:
        there is no device inflate."""
        if str(path).endswith(".gz"):
            import gzip
            with gzip.open(path, "rb") as f:
                data = f.read()
        else:
            with open(path, "rb") as f:
                data = f.read()
        return self.set_reads_text(data, 0, fmt, first_global_id)

    def export_reads(self, nreads, packed_bytes):
        packed = np.zeros(packed_bytes + 16, dtype=np.uint8); off = np.zeros(nreads, dtype=np.uint64); ln = np.zeros(nreads, dtype=np.uint32)
        self._check(self.L.elba_export_reads(self.h, packed.ctypes.data, packed_bytes, off.ctypes.data, ln.ctypes.data, nreads))
        return packed, off, ln

    def set_kmer_matrix(self, nrows, ncols, rows, cols, vals):
        rows = np.ascontiguousarray(rows, dtype=np.int64)
        cols = np.ascontiguousarray(cols, dtype=np.int64)
        vals = np.ascontiguousarray(vals, dtype=np.uint32)
        st = MatrixStats()
        self._check(self.L.elba_set_kmer_matrix(self.h, nrows, ncols, len(rows), rows.ctypes.data, cols.ctypes.data, vals.ctypes.data, C.byref(st)))
        return _stats(st)

    def set_kmer_matrix_device(self, nrows, ncols, nnz, d_rows, d_cols, d_vals):
        """The triples resident in HBM (device pointers: int64 rows, int64 cols, uint32 vals)."""
        st = MatrixStats()
        self._check(self.L.elba_set_kmer_matrix_device(self.h, nrows, ncols, nnz, d_rows, d_cols, d_vals, C.byref(st)))
        return _stats(st)

    def export_triples_device(self, d_rows, d_cols, d_vals):
        self._check(self.L.elba_export_triples_device(self.h, d_rows, d_cols, d_vals))

    def kmer_hash_owner(self, kmers, nprocs):
        """Kmer::GetHash and GetKmerOwner of the reference, computed on the device: kmers = n x W packed words."""
        km = np.ascontiguousarray(kmers, dtype=np.uint64)
        W = 3 if self.k > 64 else (2 if self.k > 32 else 1)
        n = km.size // W
        h = np.zeros(n, dtype=np.uint64); ow = np.zeros(n, dtype=np.int32)
        self._check(self.L.elba_kmer_hash_owner(self.h, km.ctypes.data if n else None, n, int(nprocs), h.ctypes.data, ow.ctypes.data))
        return h, ow

    def set_option(self, name, value):
        self._check(self.L.elba_set_option(self.h, name.encode(), int(value)))

    def get_stat(self, name):
        """a diagnostic counter of the last stage call, by name (elba_get_stat)"""
        v = C.c_int64(0)
        self._check(self.L.elba_get_stat(self.h, name.encode(), C.byref(v)))
        return int(v.value)

    def release_workspace(self):
        """the stage calls' scratch memory back to the device; matrices, reads and the multiplication's buffers stay (elba_release_workspace)"""
        self._check(self.L.elba_release_workspace(self.h))

    # --- stages ---
    def count_kmers(self):
        """get_kmer_count_map_keys + get_kmer_count_map_values."""
        st = KmerStats()
        self._check(self.L.elba_count_kmers(self.h, C.byref(st)))
        return _stats(st)

    def create_kmer_matrix(self):
        st = MatrixStats()
        self._check(self.L.elba_create_kmer_matrix(self.h, C.byref(st)))
        return _stats(st)

    def create_seed_matrix(self):
        st = OverlapStats()
        self._check(self.L.elba_create_seed_matrix(self.h, C.byref(st)))
        return _stats(st)

    def align_seeds(self, mat=1, mis=-1, gap=-1, dropoff=15):
        """PairwiseAlignment (src/PairwiseAlignment.cpp:5-106) on one rank: x-drop from seeds[0] of every stored B(i,j), i < j."""
        st = AlignStats()
        self._check(self.L.elba_align_seeds(self.h, mat, mis, gap, dropoff, C.byref(st)))
        return _stats(st)

    def export_overlaps(self):
        o = Overlaps()
        self._check(self.L.elba_export_overlaps(self.h, C.byref(o)))
        try:
            return dict(n=o.n, rows=_copy(o.rows, o.n, np.int64), cols=_copy(o.cols, o.n, np.int64), vals=_copy(o.vals, o.n, OVERLAP_DTYPE))
        finally:
            self.L.elba_free_overlaps(C.byref(o))

    # --- string graph (src/main.cpp:305-312) ---
    def set_overlaps(self, nreads, rows, cols, vals):
        """Load aligned pairs (rows < cols, ascending in (row, col)) instead of using this engine's own alignments."""
        rows = np.ascontiguousarray(rows, dtype=np.int64); cols = np.ascontiguousarray(cols, dtype=np.int64); vals = np.ascontiguousarray(vals, dtype=OVERLAP_DTYPE)
        if not (len(rows) == len(cols) == len(vals)):
            raise ValueError("set_overlaps: rows, cols, vals differ in length")
        self._check(self.L.elba_set_overlaps(self.h, int(nreads), rows.ctypes.data, cols.ctypes.data, vals.ctypes.data, len(rows)))

    def set_overlaps_device(self, nreads, d_rows, d_cols, d_vals, n):
        """set_overlaps with the three arrays in HBM (device addresses; copied device to device, checked by a kernel)."""
        self._check(self.L.elba_set_overlaps_device(self.h, int(nreads), d_rows, d_cols, d_vals, int(n)))

    def set_outside_counts(self, aligned, passed, nreads=None):
        """Attach to the loaded edge list, per read, the pairs it does not hold (u32 arrays, passed <= aligned; induce_part's outside
        counts): the next transitive_reduction counts them in its bad-read rule.  (None, None, nreads) detaches them."""
        if aligned is None or passed is None:
            self._check(self.L.elba_set_outside_counts(self.h, int(nreads or 0), None if aligned is None else np.ascontiguousarray(aligned, dtype=np.uint32).ctypes.data,
                                                       None if passed is None else np.ascontiguousarray(passed, dtype=np.uint32).ctypes.data))
            return
        aligned = np.ascontiguousarray(aligned, dtype=np.uint32); passed = np.ascontiguousarray(passed, dtype=np.uint32)
        if len(aligned) != len(passed):
            raise ValueError("set_outside_counts: aligned and passed differ in length")
        pad = np.zeros(1, dtype=np.uint32)       # (an array of 0 elements still needs an address: null means detach)
        a, p = (aligned, passed) if len(aligned) else (pad, pad)
        self._check(self.L.elba_set_outside_counts(self.h, len(aligned) if nreads is None else int(nreads), a.ctypes.data, p.ctypes.data))

    def set_outside_counts_device(self, nreads, d_aligned, d_passed):
        """set_outside_counts with the two arrays in HBM (device addresses of u32[nreads]; None, None detaches)."""
        self._check(self.L.elba_set_outside_counts_device(self.h, int(nreads), d_aligned, d_passed))

    def transitive_reduction(self, bad_read_cutoff=0.65, fuzz=1000):
        """find_bad_reads / find_contained_reads + prunes (src/main.cpp:305-311) and TransitiveReduction (src/TransitiveReduction.cpp:3-90)."""
        st = StringStats()
        self._check(self.L.elba_transitive_reduction(self.h, float(bad_read_cutoff), int(fuzz), C.byref(st)))
        d = _stats(st)
        d.pop("reserved", None)
        return d

    def export_string_graph(self):
        """Entries of S in the order parallel_write_paf walks them (columns ascending, rows ascending within a column)."""
        o = Overlaps()
        self._check(self.L.elba_export_string_graph(self.h, C.byref(o)))
        try:
            return dict(n=o.n, rows=_copy(o.rows, o.n, np.int64), cols=_copy(o.cols, o.n, np.int64), vals=_copy(o.vals, o.n, OVERLAP_DTYPE))
        finally:
            self.L.elba_free_overlaps(C.byref(o))

    def export_read_flags(self, nreads):
        """One byte per read: bit 0 = bad read, bit 1 = contained read, bit 2 = removed by clip_tips, bit 3 = removed by pop_bubbles,
        bit 4 = removed by cut_bridges, bit 5 = removed by resolve_stars."""
        f = np.zeros(int(nreads), dtype=np.uint8)
        self._check(self.L.elba_export_read_flags(self.h, f.ctypes.data, int(nreads)))
        return f

    # --- tip clipping (between transitive_reduction and generate_contigs; not in the reference) ---
    def clip_tips(self, max_tip_reads, rounds=1):
        """Removes dead-end chains of at most max_tip_reads reads that hang off a read of degree >= 3 from the string graph, in up to
        `rounds` rounds (a star of nothing but short chains is spared).  Removed reads get flag 4.  Returns the stats."""
        cfg = TipCfg(int(max_tip_reads), int(rounds), (C.c_int32 * 2)(0, 0))
        st = TipStats()
        self._check(self.L.elba_clip_tips(self.h, C.byref(cfg), C.byref(st)))
        d = _stats(st)
        d.pop("reserved", None)
        return d

    # --- bubble popping (between transitive_reduction and generate_contigs, before or after clip_tips; not in the reference) ---
    def pop_bubbles(self, max_arm_reads, rounds=1):
        """Where two or more chains of at most max_arm_reads reads of degree 2 join the same two reads of degree >= 3, keeps the one with the
        most reads (on a tie the one whose first read is smallest) and removes the others from the string graph, in up to `rounds` rounds.
        Removed reads get flag 8.  Returns the stats."""
        cfg = BubbleCfg(int(max_arm_reads), int(rounds), (C.c_int32 * 2)(0, 0))
        st = BubbleStats()
        self._check(self.L.elba_pop_bubbles(self.h, C.byref(cfg), C.byref(st)))
        d = _stats(st)
        d.pop("reserved", None)
        return d

    # --- cutting weak overlaps (between transitive_reduction and generate_contigs, before or after the two above; not in the reference) ---
    def cut_weak_overlaps(self, min_ratio=0.7):
        """Where an end of a read has two or more overlaps, removes those whose score is below min_ratio times the best score of that end
        — and every overlap that is so at its other read — from the string graph, in one pass.  Entries leave, no read does; the read
        flags stay.  min_ratio becomes min_ratio_q16 = int(round(min_ratio * 65536)), which must lie in 1 .. 65536.  Returns the stats."""
        q16 = int(round(min_ratio * 65536))
        if not 1 <= q16 <= 65536:
            raise ValueError("cut_weak_overlaps: min_ratio * 65536 rounds to %d, outside 1 .. 65536" % q16)
        cfg = WeakCfg(q16, (C.c_int32 * 3)(0, 0, 0))
        st = WeakStats()
        self._check(self.L.elba_cut_weak_overlaps(self.h, C.byref(cfg), C.byref(st)))
        return _stats(st)

    # --- cutting bridges (between transitive_reduction and generate_contigs, before or after the three above; asmtools/bridge_removal.py) ---
    def cut_bridges(self, max_bridge_reads, min_flank_reads):
        """Removes every chain of at most max_bridge_reads reads of degree 2 between two reads of degree exactly 3 whose other two edges
        each lead into at least min_flank_reads reads of degree 2 (the bar of an H), in one pass.  min_flank_reads > max_bridge_reads.
        Removed reads get flag 16; the two end reads stay, at degree 2.  Returns the stats."""
        cfg = BridgeCfg(int(max_bridge_reads), int(min_flank_reads), (C.c_int32 * 2)(0, 0))
        st = BridgeStats()
        self._check(self.L.elba_cut_bridges(self.h, C.byref(cfg), C.byref(st)))
        return _stats(st)

    # --- resolving three-armed stars (between transitive_reduction and generate_contigs, before or after the four above; asmtools/star_resolution.py) ---
    def resolve_stars(self, rounds=1):
        """A read of degree 3 whose three neighbours all have degree 2 is a centre; when exactly one pair of the three neighbours is a pair
        of R (the overlaps the last transitive_reduction started from, after its prunes), the neighbour in no such pair leaves S with its
        entries and gets flag 32.  Up to `rounds` rounds, each on the S the one before left.  Returns the stats (resolved = pairs1)."""
        cfg = StarCfg(int(rounds), (C.c_int32 * 3)(0, 0, 0))
        st = StarStats()
        self._check(self.L.elba_resolve_stars(self.h, C.byref(cfg), C.byref(st)))
        return _stats(st)

    def simplify_graph(self, max_tip_reads, max_arm_reads, passes=16, min_overlap_ratio=None, bridges=None, stars=None):
        """clip_tips(max_tip_reads, 64) then pop_bubbles(max_arm_reads, 64), again and again until a pass of both removes nothing or `passes`
        passes have run.  pop_bubbles alone does not reach that fixed point: a tip on an arm gives the arm a read of degree 3, so there is
        no arm until the tip is clipped.  (A pop makes no new tip on a symmetric graph — it lowers anchors to degree 2, which only lengthens
        dead-end chains — so the second pass is the one that finds nothing.)  Returns [(tip stats, bubble stats)], one pair per pass.
        With min_overlap_ratio every pass goes on with cut_weak_overlaps(min_overlap_ratio), which can make new dead ends and new arms: a
        pass is (tip stats, bubble stats, weak stats).  With bridges = (max_bridge_reads, min_flank_reads) every pass ends with
        cut_bridges(*bridges), whose stats are the last element of the pass's tuple.  With stars = True (64 rounds) or a round count every
        pass ends with resolve_stars, after cut_bridges if that is asked for, and its stats are the last element.  The loop ends after a
        pass in which no call removed anything."""
        out = []
        for _ in range(int(passes)):
            p = (self.clip_tips(max_tip_reads, 64), self.pop_bubbles(max_arm_reads, 64))
            idle = p[0]["reads_removed"] == 0 and p[1]["reads_removed"] == 0
            if min_overlap_ratio is not None:
                p += (self.cut_weak_overlaps(min_overlap_ratio),)
                idle = idle and p[-1]["entries_removed"] == 0
            if bridges is not None:
                p += (self.cut_bridges(*bridges),)
                idle = idle and p[-1]["reads_removed"] == 0
            if stars is not None and stars is not False:
                p += (self.resolve_stars(64 if stars is True else stars),)
                idle = idle and p[-1]["reads_removed"] == 0
            out.append(p)
            if idle:
                break
        return out

    # --- contigs (src/ContigGeneration.cpp:18-51,110,376-457, one rank) ---
    def generate_contigs(self, circular=False, singletons=False):
        """GenerateContigs on the string graph of the last transitive_reduction: branches dropped, paths walked from their smaller end.
        circular: every cycle is also walked once round from its smallest read (towards its smaller neighbour).  singletons: every read in
        no path and no cycle that is neither bad nor contained, and not empty, is also emitted, as it is.  All kinds by ascending start read."""
        st = ContigStats()
        cfg = ContigCfg((CONTIG_CIRCULAR if circular else 0) | (CONTIG_SINGLETONS if singletons else 0))
        self._check(self.L.elba_generate_contigs_ex(self.h, C.byref(cfg), C.byref(st)))
        return _stats(st)

    def export_contig_kinds(self, ncontigs):
        """One byte per contig: 0 path, 1 circular, 2 single read."""
        k = np.zeros(int(ncontigs), dtype=np.uint8)
        self._check(self.L.elba_export_contig_kinds(self.h, k.ctypes.data, int(ncontigs)))
        return k

    def export_contigs(self):
        """{n, seqs (list of str, emission order), seq_off, chain_off, chain_read, chain_prefix, chain_strand, kinds (0 path, 1 circular,
        2 single read)}."""
        o = Contigs()
        self._check(self.L.elba_export_contigs(self.h, C.byref(o)))
        try:
            n = o.n
            seq_off = _copy(o.seq_off, n + 1, np.int64)
            chain_off = _copy(o.chain_off, n + 1, np.int64)
            E = int(chain_off[-1]) if n else 0
            raw = _copy(o.seq, int(seq_off[-1]) if n else 0, np.uint8).tobytes()
            seqs = [raw[int(seq_off[i]):int(seq_off[i + 1])].decode("ascii") for i in range(n)]
            return dict(n=n, seqs=seqs, seq_off=seq_off if n else np.zeros(1, np.int64), chain_off=chain_off if n else np.zeros(1, np.int64),
                        chain_read=_copy(o.chain_read, E, np.int64), chain_prefix=_copy(o.chain_prefix, E, np.int32), chain_strand=_copy(o.chain_strand, E, np.uint8),
                        kinds=self.export_contig_kinds(n))
        finally:
            self.L.elba_free_contigs(C.byref(o))

    def export_read_contigs(self, nreads):
        """Contig index of every read of the graph; -1 for the reads in none (by default: branches, isolated reads and reads on cycles)."""
        out = np.zeros(int(nreads), dtype=np.int64)
        self._check(self.L.elba_export_read_contigs(self.h, out.ctypes.data, int(nreads)))
        return out

    def assembly_links(self):
        """The links of the assembly graph over the contigs of the last generate_contigs (include/elba_amd.h states the rule): the edges
        of S at branch reads as (from contig, orientation, to contig, orientation, overlap), plus one closure record per circular contig.
        Returns (records as a LINK_DTYPE array sorted by (from_read, to_read), stats dict).  formats.write_gfa writes them."""
        o, st = Links(), GraphStats()
        self._check(self.L.elba_export_assembly_links(self.h, C.byref(o), C.byref(st)))
        try:
            links = _copy(o.links, int(o.n), LINK_DTYPE)
        finally:
            self.L.elba_free_links(C.byref(o))
        out = _stats(st)
        del out["reserved"]
        return links, out

    def graph_components(self, graph="string", bases=False, flags=None, reserved=(0, 0)):
        """Connected components of the string graph ("string") or of the overlap graph ("overlaps": the passed pairs of the graph's
        input); include/elba_amd.h states the rule.  Every read gets one; components are numbered by ascending smallest read.  Returns
        ({comp_of_read (i32[nreads]), first_read, reads, bases, edges, branches, ends (i64[n])}, stats dict); bases is all zero without
        bases=True, which needs the reads' lengths on the context.  formats.write_gfa(component=) and write_contigs_fasta(components=)
        take a contig's component: that of its first chain read."""
        g = _CC_GRAPHS.get(graph, graph) if isinstance(graph, str) else graph
        if isinstance(g, str):
            raise ValueError("graph_components: graph is 'string' or 'overlaps'")
        fl = (CC_BASES if bases else 0) if flags is None else int(flags)
        cfg = CcCfg(int(g), fl, (C.c_int32 * 2)(*[int(x) for x in reserved]))
        o, st = Components(), CcStats()
        self._check(self.L.elba_graph_components(self.h, C.byref(cfg), C.byref(o), C.byref(st)))
        try:
            M, n = int(o.nreads), int(o.n)
            cc = dict(comp_of_read=_copy(o.comp_of_read, M, np.int32))
            for name in ("first_read", "reads", "bases", "edges", "branches", "ends"):
                cc[name] = _copy(getattr(o, name), n, np.int64)
        finally:
            self.L.elba_free_components(C.byref(o))
        out = _stats(st)
        del out["reserved"]
        return cc, out

    def partition_components(self, nparts, graph="string", weight="reads", min_reads=2, nreads=None, reserved=(0, 0, 0, 0)):
        """The reference's greedy assignment of components to `nparts` parts, made deterministic (include/elba_amd.h): the components of
        at least min_reads reads, heaviest first (weight "reads" or "bases"), each to the part with the smallest sum so far.  The call
        labels the graph itself.  Returns (part_of_read (i32[nreads], -1: a read of a smaller component), part_weight (i64[nparts]))."""
        g = _CC_GRAPHS.get(graph, graph) if isinstance(graph, str) else graph
        w = _CC_WEIGHTS.get(weight, weight) if isinstance(weight, str) else weight
        if isinstance(g, str) or isinstance(w, str):
            raise ValueError("partition_components: graph is 'string' or 'overlaps', weight is 'reads' or 'bases'")
        cfg = PartCfg(int(g), int(nparts), int(w), int(min_reads), (C.c_int32 * 4)(*[int(x) for x in reserved]))
        if nreads is None:
            nreads = self.graph_components(graph=int(g))[1]["nreads"]
        part = np.full(max(int(nreads), 1), -1, dtype=np.int32)
        pw = np.zeros(max(int(nparts), 1), dtype=np.int64)
        self._check(self.L.elba_partition_components(self.h, C.byref(cfg), part.ctypes.data, int(nreads), pw.ctypes.data))
        return part[:int(nreads)], pw[:max(int(nparts), 0)]

    def induce_part(self, part_of_read, part, bases=True, host=True, flags=None, reserved=(0, 0)):
        """The induced sub-problem of one part (elba_induce_part; include/elba_amd.h states the rule): the reads v of the graph's input with
        part_of_read[v] == part, renumbered in order, the pairs between them, and per new read the pairs that leave the part.  Returns
        (dict, stats): reads, pairs, packed_bytes, the device addresses d_* (valid until the next induce_part, release_workspace or
        close) and, with host=True, numpy copies old_of_new, rows, cols, vals, outside_aligned, outside_passed and — with bases=True —
        packed (with its 16 guard bytes), byte_off, len.  Engine.load_part(dict) loads it into an engine."""
        pr = np.ascontiguousarray(part_of_read, dtype=np.int32)
        fl = ((INDUCE_BASES if bases else 0) | (INDUCE_HOST if host else 0)) if flags is None else int(flags)
        cfg = InduceCfg(int(part), fl, (C.c_int32 * 2)(*[int(x) for x in reserved]))
        o, st = Induced(), InduceStats()
        pad = np.zeros(1, dtype=np.int32)
        self._check(self.L.elba_induce_part(self.h, C.byref(cfg), pr.ctypes.data if len(pr) else pad.ctypes.data, len(pr), C.byref(o), C.byref(st)))
        try:
            R, P, pb = int(o.reads), int(o.pairs), int(o.packed_bytes)
            ind = dict(reads=R, pairs=P, packed_bytes=pb)
            for name in ("d_old_of_new", "d_packed", "d_byte_off", "d_len", "d_rows", "d_cols", "d_vals", "d_outside_aligned", "d_outside_passed"):
                ind[name] = getattr(o, name)
            if o.old_of_new:
                ind.update(old_of_new=_copy(o.old_of_new, R, np.int64), rows=_copy(o.rows, P, np.int64), cols=_copy(o.cols, P, np.int64), vals=_copy(o.vals, P, OVERLAP_DTYPE),
                           outside_aligned=_copy(o.outside_aligned, R, np.uint32), outside_passed=_copy(o.outside_passed, R, np.uint32))
                if o.packed:
                    ind.update(packed=_copy(o.packed, pb + 16, np.uint8), byte_off=_copy(o.byte_off, R, np.uint64), len=_copy(o.len, R, np.uint32))
        finally:
            self.L.elba_free_induced(C.byref(o))
        return ind, _stats(st)

    def load_part(self, ind, outside=True):
        """Load the host copies of an induce_part result into THIS engine: set_reads (when the part carries bases) + set_overlaps +
        set_outside_counts.  outside=False leaves the counts out (what a driver without them computes: no guarantee)."""
        if "rows" not in ind:
            raise ValueError("load_part: the part has no host copies (induce_part(host=True))")
        if "packed" in ind:
            self.set_reads(ind["packed"], ind["byte_off"], ind["len"])
        self.set_overlaps(ind["reads"], ind["rows"], ind["cols"], ind["vals"])
        if outside:
            self.set_outside_counts(ind["outside_aligned"], ind["outside_passed"], nreads=ind["reads"])

    def place_reads(self, skip_flags=1, reserved=(0, 0, 0)):
        """Every read on its contig and the depth of every contig base (include/elba_amd.h states the rule): chain reads where the contig
        stage put them, every other read that has none of `skip_flags` in its read flags through its best-scoring passed pair with a
        chain read.  Returns ({reads (PLACEMENT_DTYPE, one per read), seg_off (i64[ncontigs + 1]), seg_start, seg_depth (i32),
        credited_reads, credited_bases (i64[ncontigs])}, stats dict).  formats.write_placements_paf and write_gfa(depth=) take them."""
        cfg = PlaceCfg(int(skip_flags), (C.c_int32 * 3)(*[int(x) for x in reserved]))
        o, st = Placements(), PlaceStats()
        self._check(self.L.elba_place_reads(self.h, C.byref(cfg), C.byref(o), C.byref(st)))
        try:
            M, nc = int(o.nreads), int(o.ncontigs)
            seg_off = _copy(o.seg_off, nc + 1, np.int64)
            S = int(seg_off[-1])
            pl = dict(reads=_copy(o.reads, M, PLACEMENT_DTYPE), seg_off=seg_off, seg_start=_copy(o.seg_start, S, np.int32), seg_depth=_copy(o.seg_depth, S, np.int32),
                      credited_reads=_copy(o.credited_reads, nc, np.int64), credited_bases=_copy(o.credited_bases, nc, np.int64))
        finally:
            self.L.elba_free_placements(C.byref(o))
        out = _stats(st)
        del out["reserved"]
        return pl, out

    def polish_contigs(self, skip_flags=1, band=64, max_diff=0.25, min_depth=3, votes=False, flags=None, reserved=(0, 0, 0), max_diff_q16=None):
        """The contigs of the last generate_contigs with every column and gap voted on by the reads placed there (include/elba_amd.h states
        the rule): place_reads' records under `skip_flags`, a banded edit-distance alignment of every placed read (band 64, 128 or 256
        diagonals; a read with more than max_diff differences per base does not vote), columns with fewer than min_depth votes kept.
        Returns ({seqs (list of str, the order of export_contigs), seq_off, voters, substituted, deleted, inserted (i64[ncontigs])}, stats
        dict); with votes=True also col_off, col (u32[bases, 5]), gap (u32[bases + ncontigs, 4]: contig k's gap g at row col_off[k] + k + g)
        and reads (POLISH_READ_DTYPE, one per read).  formats.write_contigs_fasta takes seqs as it takes export_contigs' ones."""
        q16 = int(round(float(max_diff) * 65536)) if max_diff_q16 is None else int(max_diff_q16)
        fl = (POLISH_EXPORT_VOTES if votes else 0) if flags is None else int(flags)
        cfg = PolishCfg(int(skip_flags), int(band), q16, int(min_depth), fl, (C.c_int32 * 3)(*[int(x) for x in reserved]))
        o, st = Polished(), PolishStats()
        self._check(self.L.elba_polish_contigs(self.h, C.byref(cfg), C.byref(o), C.byref(st)))
        try:
            n = int(o.n)
            seq_off = _copy(o.seq_off, n + 1, np.int64)
            raw = _copy(o.seq, int(seq_off[-1]) if n else 0, np.uint8).tobytes()
            out = dict(seqs=[raw[int(seq_off[i]):int(seq_off[i + 1])].decode("ascii") for i in range(n)], seq_off=seq_off if n else np.zeros(1, np.int64),
                       voters=_copy(o.voters, n, np.int64), substituted=_copy(o.substituted, n, np.int64), deleted=_copy(o.deleted, n, np.int64),
                       inserted=_copy(o.inserted, n, np.int64))
            if fl & POLISH_EXPORT_VOTES:
                col_off = _copy(o.col_off, n + 1, np.int64) if n else np.zeros(1, np.int64)
                bases = int(col_off[-1])
                out.update(col_off=col_off, col=_copy(o.col, 5 * bases, np.uint32).reshape(bases, 5), gap=_copy(o.gap, 4 * (bases + n), np.uint32).reshape(bases + n, 4),
                           reads=_copy(o.reads, int(o.nreads), POLISH_READ_DTYPE))
        finally:
            self.L.elba_free_polished(C.byref(o))
        return out, _stats(st)

    # --- read pileups and chimera flags (src/PruneChimeras.cpp; after align_seeds, before transitive_reduction) ---
    def read_pileup(self, mode=0, margin=0, min_depth=1, min_run=1, trim_len=2500):
        """Per-read coverage from the pairs transitive_reduction would read (both reads of a pair credited), the trimmed interval by
        GetTrimmedInterval's rule (best run returned) and the flags (bit 0 unsupported, bit 1 split).  Returns the stats."""
        cfg = PileupCfg(int(mode), int(margin), int(min_depth), int(min_run), int(trim_len), 0)
        st = PileupStats()
        self._check(self.L.elba_read_pileup(self.h, C.byref(cfg), C.byref(st)))
        d = _stats(st)
        d.pop("reserved", None)
        return d

    def export_pileup(self):
        """{n, seg_off (i64[n+1]), seg_start, seg_depth (i32), trim_beg, trim_end (i32[n]), flags (u8[n])}."""
        o = Pileup()
        self._check(self.L.elba_export_pileup(self.h, C.byref(o)))
        try:
            n, S = o.n, o.nseg
            return dict(n=n, seg_off=_copy(o.seg_off, n + 1, np.int64), seg_start=_copy(o.seg_start, S, np.int32), seg_depth=_copy(o.seg_depth, S, np.int32),
                        trim_beg=_copy(o.trim_beg, n, np.int32), trim_end=_copy(o.trim_end, n, np.int32), flags=_copy(o.flags, n, np.uint8))
        finally:
            self.L.elba_free_pileup(C.byref(o))

    def prune_reads(self, mask):
        """PruneFull of the reads with flags & mask: the kept pairs become the edge list transitive_reduction reads next.  Returns their count."""
        kept = C.c_int64(0)
        self._check(self.L.elba_prune_reads(self.h, int(mask), C.byref(kept)))
        return int(kept.value)

    # --- reads cut to their supported intervals (after read_pileup; adopt_trimmed_reads starts the pipeline again on the pieces) ---
    def trim_reads(self, mode=0, min_len=1, reserved=(0, 0)):
        """mode 0: one piece per read, its trimmed interval; mode 1: one piece per long run of the last read_pileup (a chimera is split).
        Pieces shorter than min_len are dropped.  The new read set stays on the device.  Returns the stats."""
        cfg = TrimCfg(int(mode), int(min_len), (C.c_int32 * 2)(int(reserved[0]), int(reserved[1])))
        st = TrimStats()
        self._check(self.L.elba_trim_reads(self.h, C.byref(cfg), C.byref(st)))
        return _stats(st)

    def export_trim_map(self):
        """{n, src_read (i64[n]), src_beg, src_end (i32[n])}: piece p is bases [src_beg, src_end) of read src_read; (src_read, src_beg) ascending."""
        o = TrimMap()
        self._check(self.L.elba_export_trim_map(self.h, C.byref(o)))
        try:
            n = o.n
            return dict(n=n, src_read=_copy(o.src_read, n, np.int64), src_beg=_copy(o.src_beg, n, np.int32), src_end=_copy(o.src_end, n, np.int32))
        finally:
            self.L.elba_free_trim_map(C.byref(o))

    def trimmed_reads_device(self):
        """{d_packed, packed_bytes, d_byte_off (u64[n]), d_len (u32[n]), n}: device addresses of the trimmed read set (DnaBuffer layout, 16
        zeroed guard bytes behind packed_bytes), valid until the next trim_reads, adopt_trimmed_reads or close."""
        dp, do, dl = C.c_void_p(), C.c_void_p(), C.c_void_p()
        pb, n = C.c_int64(0), C.c_int64(0)
        self._check(self.L.elba_get_trimmed_reads_device(self.h, C.byref(dp), C.byref(pb), C.byref(do), C.byref(dl), C.byref(n)))
        return dict(d_packed=dp.value, packed_bytes=int(pb.value), d_byte_off=do.value, d_len=dl.value, n=int(n.value))

    def export_trimmed_reads(self):
        """Host copies (packed with its 16 guard bytes, byte_off u64, len u32) of the trimmed read set; the snapshot stays on the device."""
        v = self.trimmed_reads_device()
        return (_copy_from_device(v["d_packed"], v["packed_bytes"] + 16, np.uint8), _copy_from_device(v["d_byte_off"], v["n"], np.uint64),
                _copy_from_device(v["d_len"], v["n"], np.uint32))

    def adopt_trimmed_reads(self):
        """The pieces become this context's reads, exactly as after set_reads (everything derived from the old reads is invalidated)."""
        self._check(self.L.elba_adopt_trimmed_reads(self.h))

    # --- outputs ---
    def export_csr(self, row_lo=0, row_hi=None):
        if row_hi is None:
            row_hi = self.device_view()["M"]
        o = Csr()
        self._check(self.L.elba_export_csr(self.h, row_lo, row_hi, C.byref(o)))
        try:
            return dict(M=o.nrows, Y=o.nnz, rowptr=_copy(o.rowptr, o.nrows + 1, np.int64), col=_copy(o.col, o.nnz, np.int64), val=_copy(o.val, o.nnz, SEED_DTYPE))
        finally:
            self.L.elba_free_csr(C.byref(o))

    def export_dcsc(self, row_lo, row_hi, col_lo, col_hi):
        o = Dcsc()
        self._check(self.L.elba_export_dcsc(self.h, row_lo, row_hi, col_lo, col_hi, C.byref(o)))
        try:
            return dict(nnz=o.nnz, nzc=o.nzc, jc=_copy(o.jc, o.nzc, np.int64), cp=_copy(o.cp, o.nzc + 1, np.int64),
                        ir=_copy(o.ir, o.nnz, np.int64), numx=_copy(o.numx, o.nnz, SEED_DTYPE))
        finally:
            self.L.elba_free_dcsc(C.byref(o))

    def export_kmer_matrix(self):
        o = KmerMatrix()
        self._check(self.L.elba_export_kmer_matrix(self.h, C.byref(o)))
        try:
            return dict(M=o.nrows, N=o.ncols, Z=o.nnz, kmers=_copy(o.kmers, o.ncols, np.uint64) if o.kmers else None,
                        kmers_lo=_copy(o.kmers_lo, o.ncols, np.uint64) if o.kmers_lo else None,
                        kmers_lo2=_copy(o.kmers_lo2, o.ncols, np.uint64) if o.kmers_lo2 else None,
                        colptr=_copy(o.colptr, o.ncols + 1, np.int64), csc_read=_copy(o.csc_row, o.nnz, np.int64), csc_pos=_copy(o.csc_val, o.nnz, np.uint32),
                        rowptr=_copy(o.rowptr, o.nrows + 1, np.int64), csr_kid=_copy(o.csr_col, o.nnz, np.int64), csr_pos=_copy(o.csr_val, o.nnz, np.uint32))
        finally:
            self.L.elba_free_kmer_matrix(C.byref(o))

    def kmer_histogram(self, n=None):
        n = n or self.upper + 2
        h = np.zeros(n, dtype=np.int64)
        self._check(self.L.elba_kmer_histogram(self.h, h.ctypes.data, n))
        return h

    def device_view(self):
        v = DeviceView()
        self._check(self.L.elba_get_device_view(self.h, C.byref(v)))
        return _stats(v)
