/*
 * elba_amd.h — C ABI of the MI355X-native overlap-detection engine (libelba_amd.so).
 *
 * This is the drop-in boundary for ELBA's hot path.  Each entry point names the
 * reference interface it replaces; all file:line citations are into PASSIONLab/ELBA @ v2.
 *
 *   reference (C++/MPI/CombBLAS, one call chain in src/main.cpp:191-285)      this ABI
 *   -----------------------------------------------------------------------   --------------------------------
 *   DnaBuffer (include/DnaBuffer.hpp:13-38), index.getmydna() main.cpp:126      elba_set_reads / elba_set_reads_device
 *   get_kmer_count_map_keys   (include/KmerOps.hpp:27-28, main.cpp:192)   \
 *   get_kmer_count_map_values (include/KmerOps.hpp:30,    main.cpp:225)   /    elba_count_kmers
 *   create_kmer_matrix        (include/KmerOps.hpp:24-25, main.cpp:259)   \
 *   AT = *A; AT->Transpose()  (src/main.cpp:272-273)                      /    elba_create_kmer_matrix
 *   (A handed over by a caller that already owns it: the SpParMat triples
 *    of src/KmerOps.cpp:380-400)                                               elba_set_kmer_matrix
 *   create_seed_matrix        (include/SharedSeeds.hpp:98-99, main.cpp:281)    elba_create_seed_matrix
 *   Bmat.seqptr()->GetDCSC()  (src/PairwiseAlignment.cpp:16-19)                elba_export_dcsc
 *   SharedSeeds               (include/SharedSeeds.hpp:8-96)                   elba_seed_t
 *
 * Conventions: plain pointers and sizes only; every function returns an int status (ELBA_OK == 0);
 * host arrays handed in are borrowed for the duration of the call; arrays handed out are owned by
 * the library and released with the matching elba_free_* call.  One context per process and GPU,
 * calls on a context are serialised by the caller (the reference is single-threaded per rank on this
 * path).  The library fails loudly (ELBA_ERR_NO_DEVICE) when no HIP device is present:
 * there is no CPU fallback.
 *
 * Canonical result order: k-mer ids are the ranks of the packed canonical k-mer
 * values (ascending); entries of a column of A are ordered by (read, pos), of a row by (k-mer id, pos);
 * B(i,j).seeds[0] / seeds[1] are the products with minimal / maximal (k-mer id, posQ, posT) — what an
 * ascending-k left fold of SharedSeeds::Semiring::add (include/SharedSeeds.hpp:41-46) yields.
 */
#ifndef ELBA_AMD_H_
#define ELBA_AMD_H_

#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ELBA_ABI_VERSION 3

enum {
    ELBA_OK = 0,
    ELBA_ERR_INVALID_ARG   = 1,  /* bad pointer / size / (k, lower, upper) outside include/compiletime.h:10,21 */
    ELBA_ERR_NO_DEVICE     = 2,  /* no HIP device: the product path has no CPU fallback */
    ELBA_ERR_HIP           = 3,  /* a HIP runtime call failed (elba_last_error has the text) */
    ELBA_ERR_OUT_OF_MEMORY = 4,
    ELBA_ERR_STATE         = 5,  /* stage called before its inputs exist */
    ELBA_ERR_UNSUPPORTED   = 6,  /* k outside 3..95, index ranges beyond 32 bit, LOWER == 1 */
    ELBA_ERR_INTERNAL      = 7,
    ELBA_ERR_RETRY         = 8   /* elba_seed_matrix_recv: some rank ran out of room; every rank got this answer: repeat the step */
};

typedef struct elba_ctx elba_ctx;

/* SharedSeeds with an explicit field order (the reference's std::tuple pair is laid out reversed in
 * memory, SURVEY.md a11 — never memcpy into it, use std::get<>). */
typedef struct { uint32_t q0, t0, q1, t1; int32_t numshared; } elba_seed_t;

/* The fields of the reference's Overlap that Overlap::extend_overlap fills (include/Overlap.hpp:22-28, src/Overlap.cpp:24-73),
 * explicit order (beg/end are std::tuples in the reference: same caveat as above), plus the OverlapClass it was derived from. */
typedef struct {
    int32_t begQ, begT, endQ, endT;     /* beg = (begQ, begT), end = (endQ, endT) */
    int32_t score, suffix, suffixT;
    int8_t  direction, directionT;      /* -1 = none */
    uint8_t rc, passed, containedQ, containedT;
    uint8_t kind;                       /* OverlapClass: 0 BAD_ALIGNMENT, 1 FIRST_CONTAINED, 2 SECOND_CONTAINED, 3 FIRST_TO_SECOND_OVERLAP, 4 SECOND_TO_FIRST_OVERLAP */
    uint8_t reserved;
} elba_overlap_t;

/* One line of the samtools-style .fai next to the FASTA: FastaIndex::Record (include/FastaIndex.hpp:10; name and line width with
 * newline are not kept by the reference either: src/FastaIndex.cpp:15-23 reads `name len pos bases`). */
typedef struct { uint64_t len, pos, bases; } elba_fasta_record_t;

typedef struct {
    int64_t nreads, bases, packed_bytes, chunk_bytes;
    float   ms_total;       /* H2D copy of the chunk + encode */
    float   ms_encode;      /* the encode kernel alone */
} elba_ingest_stats;

typedef struct {
    int64_t nalignments;    /* candidate pairs aligned: stored B(i,j) with i < j (src/PairwiseAlignment.cpp:52 on one rank) */
    int64_t seeds_rejected; /* xdrop_aligner returned -1 (src/XDropAligner.cpp:231-245) */
    int64_t passed;         /* Overlap::passed */
    int64_t contained;      /* containedQ or containedT */
    int64_t extensions_strided; /* extensions whose band outgrew one wavefront (redone by the strided kernel) */
    int64_t cells;          /* DP cells computed (both extensions of every pair) — the unit of the stage's throughput */
    float   ms_total;       /* device time of the stage */
    float   ms_extend;      /* the extension kernels (dominant) */
} elba_align_stats;

/* rows[a], cols[a] (global read ids) and vals[a] of the a-th aligned pair, in CSR order of B's strict upper triangle:
 * the triples PairwiseAlignment hands to SpParMat<Overlap> (src/PairwiseAlignment.cpp:97-103). */
typedef struct {
    int64_t n;
    int64_t *rows, *cols;
    elba_overlap_t *vals;
} elba_overlaps_t;

/* From the aligned pairs to the string graph (src/main.cpp:305-312). */
typedef struct {
    int64_t nreads, nedges;     /* reads, aligned pairs handed in (entries of the upper-triangular R of PairwiseAlignment) */
    int64_t bad_reads;          /* find_bad_reads (src/main.cpp:553-571) */
    int64_t edges_passed;       /* entries left by Prune(!passed) + PruneFull(bad reads) */
    int64_t contained_reads;    /* find_contained_reads (src/main.cpp:573-583) */
    int64_t edges_kept;         /* entries left by PruneFull(contained reads): the R handed to TransitiveReduction (upper triangle) */
    int64_t products;           /* semiring products of R (x) R on the symmetrised R = sum over reads of degree^2: lookups done */
    int64_t marked;             /* nnz(I) before it is symmetrised: entries of R with suffix + FUZZ >= the two-edge path of their direction */
    int64_t removed;            /* nnz(T) */
    int64_t nnz;                /* nnz(S): both triangles */
    int32_t iterations;         /* passes of the reference's do-while this stands for (2 when something was removed, else 1; see tr.hip) */
    int32_t reserved;
    float   ms_total;           /* device time of the stage */
    float   ms_minplus;         /* the masked min-plus kernel alone */
} elba_string_stats;

typedef struct {
    int32_t k;          /* KMER_SIZE: odd, 3..95 as in the reference (one to three 64-bit words per k-mer; reference: compile-time, Makefile:1) */
    int32_t lower;      /* LOWER_KMER_FREQ >= 2 (SURVEY.md App. A.4 precondition)            */
    int32_t upper;      /* UPPER_KMER_FREQ <= 65535                                          */
    int32_t device;     /* HIP device ordinal                                                */
    int64_t workspace_hint_bytes; /* 0 = decide from the input; otherwise pre-size the overlap workspace */
    int32_t flags;      /* reserved, 0 */
    int32_t timing_stride; /* elba_create_seed_matrix records its phase events (ms_* of elba_overlap_stats) on every timing_stride-th
                              steady-state call only; 0 or 1 = every call.  An event record costs ~5 us of stream time on a ~0.25 ms call:
                              a caller that does not read the phase times every call should not pay for them every call. */
} elba_cfg;

typedef struct {
    int64_t nreads;        /* M                                                       */
    int64_t instances;     /* I  = sum_reads max(0, len-k+1)                          */
    int64_t distinct;      /* distinct canonical k-mers seen                          */
    int64_t reliable;      /* N  = k-mers with lower <= count <= upper                */
    int64_t entries;       /* Z  = nnz(A)                                             */
    float   ms_total;      /* device time of the stage (HIP events on the library's stream) */
    float   ms_count;      /* "collecting distinct k-mers": enumerate + value partition (k <= 31), or enumerate + sort */
    float   ms_lookup;     /* unused (0): there is no second enumeration — an instance carries its read and position */
    float   ms_sort;       /* "counting recording k-mer seeds": per-bucket exact count, [lower, upper] filter, columns */
} elba_kmer_stats;

typedef struct {
    int64_t nrows, ncols, nnz;   /* M, N, Z */
    int64_t max_row_nnz;
    float   ms_total;
} elba_matrix_stats;

typedef struct {
    int64_t nrows;          /* M */
    int64_t products;       /* P = sum_k c_k^2 (semiring multiplies)                      */
    int64_t nnz_before_prune; /* Y_raw = nnz of the raw product                            */
    int64_t nnz;            /* Y = nnz(B) after Prune(numshared <= 1) — the metric's unit */
    int64_t nnz_diag;       /* diagonal entries kept                                      */
    int64_t nnz_upper;      /* strict upper triangle = #alignment candidates on one rank  */
    int64_t max_numshared;
    int64_t rows_lds;       /* rows accumulated in LDS tables                             */
    int64_t rows_global;    /* rows spilled to the HBM table path                         */
    int64_t rows_escalated; /* optimistic-table overflows re-queued on a larger tier      */
    int64_t algorithmic_bytes; /* 16Z + 8(2M+N+3) + 24Y                    */
    int32_t passes;         /* 1, or 2 when the output workspace had to grow              */
    int32_t timed;          /* 1: ms_* below were measured in this call; 0: this call recorded no events (cfg.timing_stride), ms_* are 0 */
    float   ms_total;       /* whole timed region: resident A -> resident pruned CSR B    */
    float   ms_symbolic;    /* row upper bounds + binning                                 */
    float   ms_numeric;     /* hash-accumulate kernels (the dominant kernels)             */
    float   ms_finalize;    /* row-pointer scan + per-row column sort + copy              */
} elba_overlap_stats;

/* CombBLAS-shaped DCSC of a block of B with LOCAL indices: exactly the arrays walked by
 * src/PairwiseAlignment.cpp:28-32 (jc[nzc], cp[nzc+1], ir[nnz], numx[nnz]). */
typedef struct {
    int64_t nrows, ncols, nnz, nzc;
    int64_t *jc, *cp, *ir;
    elba_seed_t *numx;
} elba_dcsc_t;

/* B (or a row range of it) as CSR, columns ascending within a row. */
typedef struct {
    int64_t nrows, ncols, nnz;
    int64_t *rowptr;       /* [nrows+1] */
    int64_t *col;          /* [nnz]     */
    elba_seed_t *val;      /* [nnz]     */
} elba_csr_t;

/* A in both orientations, for parity checks and for callers that want CombBLAS triples back. */
typedef struct {
    int64_t nrows, ncols, nnz;
    uint64_t *kmers;       /* [ncols] packed canonical k-mer of each column (NULL if A came from elba_set_kmer_matrix); first word */
    uint64_t *kmers_lo;    /* [ncols] second word (bases 32..63, left-aligned) when k > 32, else NULL */
    uint64_t *kmers_lo2;   /* [ncols] third word (bases 64..k-1) when k > 64, else NULL */
    int64_t *colptr;       /* [ncols+1] */
    int64_t *csc_row;      /* [nnz] read id, within a column ordered by (read, pos) */
    uint32_t *csc_val;     /* [nnz] position */
    int64_t *rowptr;       /* [nrows+1] */
    int64_t *csr_col;      /* [nnz] k-mer id, within a row ordered by (kid, pos) */
    uint32_t *csr_val;     /* [nnz] position */
} elba_kmer_matrix_t;

/* Device-resident views (HIP pointers, valid until the next stage call / destroy): for consumers that stay on the GPU
 * (next rows f1/f2 of SURVEY.md §8f) and for the benchmark harness. */
typedef struct {
    int64_t M, N, Z, Y;
    const void *a_rowptr;  /* u32[M+1] */
    const void *a_csr;     /* u64[Z]: kid<<32 | hint<<30 | pos: positions below 2^30 (else hint = 0 and pos takes 32 bits); hint = two ownership bits
                              the SpGEMM reads (an entry whose row accumulates no pair of its column skips the column).  Dense matrices (a column longer than 16
                              entries, positions below 2^16): kid<<32 | column length<<23 | the entry's place in its column<<16 | pos.
                              elba_export_kmer_matrix returns plain positions */
    const void *a_colptr;  /* u32[N+1] */
    const void *a_csc;     /* u64[Z]: read<<32 | pos */
    const void *b_rowptr;  /* i64[M+1] */
    const void *b_col;     /* u32[Y] */
    const void *b_val;     /* elba_seed_t[Y] */
    void *stream;          /* hipStream_t the library launches on */
    uint32_t a_csr_format; /* which of the four encodings of a_csr is active (ELBA_CSR_*) */
    uint32_t a_csr_pos_mask; /* position of an a_csr entry = low word & a_csr_pos_mask, whatever the format */
    const void *a_kmers;   /* u64[N]: packed canonical k-mer (first word) of every column, ascending; NULL when A came from triples */
    int64_t a_gather_slots;/* ELBA_CSR_INLINE matrices built by elba_count_kmers: > 0 = an a_csr entry WITHOUT bit 63 and with hint == 0 (an entry that
                              fetches its column) names its column's gather slot in the id field, not the k-mer id; a_slot_kid maps back.  0: ids are k-mer ids */
    const void *a_slot_kid;/* u32[a_gather_slots]: k-mer id of every gather slot (slots are drawn in chunks: unused ones hold garbage) */
} elba_device_view;
enum { ELBA_CSR_PLAIN = 0 /* kid<<32 | pos */, ELBA_CSR_HINTS = 1 /* kid<<32 | hint<<30 | pos */, ELBA_CSR_DENSE = 2 /* kid<<32 | L<<23 | idx<<16 | pos */,
       ELBA_CSR_INLINE = 3 /* as HINTS, but an entry with bit 63 set carries the one partner of its two-read column instead of the k-mer id:
                              1<<63 | (partner>>1)<<32 | pos | partner's pos<<16 (positions below 2^16; the partner's low bit follows from the
                              ownership rule: DESIGN.md §4.1).  elba_export_kmer_matrix and the column side (a_colptr / a_csc / a_kmers) stay canonical */ };

int  elba_abi_version(void);
const char *elba_strerror(int status);
const char *elba_last_error(const elba_ctx *ctx);           /* detail text of the last failure on this context */

int  elba_ctx_create(elba_ctx **out, const elba_cfg *cfg);
void elba_ctx_destroy(elba_ctx *ctx);

/* DnaBuffer layout (src/DnaSeq.cpp:7-29, src/DnaBuffer.cpp:22-29): read r occupies bytes
 * [byte_off[r], byte_off[r] + (len[r]+3)/4) of `packed`, 4 bases per byte, first base in bits 7-6.
 * first_global_id: global id of local read 0 (the reference's MPI_Exscan offset, src/KmerOps.cpp:215). */
int  elba_set_reads(elba_ctx *ctx, const uint8_t *packed, const uint64_t *byte_off, const uint32_t *len,
                    int64_t nreads, int64_t first_global_id);
/* Same, with all three arrays already resident in HBM on cfg.device (no copy; caller keeps them alive). */
int  elba_set_reads_device(elba_ctx *ctx, const void *d_packed, int64_t packed_bytes, const void *d_byte_off,
                           const void *d_len, int64_t nreads, int64_t first_global_id);

/* FastaIndex::getmydna (src/FastaIndex.cpp:191-290) without the host-side parse: `chunk` holds the raw bytes of the FASTA file from
 * file offset `chunk_file_offset` on (the reference's MPI_File_read_at_all buffer, :236-241), `recs` the .fai records of this rank's
 * reads in order; the reads are 2-bit encoded on the device straight into the DnaBuffer layout (DnaSeq::compress, src/DnaSeq.cpp:7-29)
 * and become the context's reads, as after elba_set_reads. */
int  elba_set_reads_fasta(elba_ctx *ctx, const char *chunk, int64_t chunk_bytes, uint64_t chunk_file_offset,
                          const elba_fasta_record_t *recs, int64_t nreads, int64_t first_global_id, elba_ingest_stats *stats);
/* Reads from raw FASTA or FASTQ text, without a .fai: the index is built on the device (elba_amd/csrc/text_index.hip) and
 * the call ends where elba_set_reads_fasta ends — the reads 2-bit encoded (the same kernel: N/n as A, any other character code 4 ORed in
 * truncated to 8 bits) as the context's own, in DnaBuffer layout.  `chunk` = chunk_bytes bytes of the file from offset chunk_file_offset
 * on, beginning at a record; cfg NULL = ELBA_TEXT_AUTO (first byte '>' FASTA, '@' FASTQ; an empty chunk: FASTA, no reads), first id 0.
 * Lines end at '\n'.  FASTA: a line that begins with '>' starts a record; pos = the offset behind the header's newline (the chunk's end
 * when there is none), len = the record's bytes without its newlines, bases = the length of its first sequence line (1 when len is 0);
 * the line lengths of a record must read bases, .., bases, t, 0, .., 0 with 0 <= t <= bases (trailing empty lines are allowed, a blank
 * line in the middle is not).  FASTQ: four lines per record — '@' header, sequence, '+' line, quality of the sequence's length; the
 * rank of a line decides its role, quality values are not kept, bases = max(len, 1).  A name begins behind the '>' / '@' and ends at the
 * first space, tab, VT, FF or the line's end.  ELBA_ERR_INVALID_ARG: a '\r' anywhere, a first byte that is neither '>' nor '@', a line
 * that breaks the shape, a FASTQ line count that is no multiple of 4, a missing '@' or '+', a quality line of another length, a read of
 * 0x7FFFFFF0 bases or more — of several violations the one with the smallest file offset is reported (the offending byte for '\r', the
 * line's start otherwise, the record's header for a quality length), and elba_last_error names its kind, record and file offset.
 * ELBA_ERR_UNSUPPORTED: 2^32-1 lines or reads, or more.  A rejected call leaves the previous reads and their index in place; as a
 * rejected elba_set_reads_fasta, it still invalidates the pileup and the trimmed reads.
 * elba_export_read_index: the .fai records and the name extents of the reads (pos and name_pos are file offsets, chunk_file_offset
 * included; caller-allocated arrays of nreads_capacity >= nreads entries, any pointer may be NULL).  The index belongs to the read set:
 * ELBA_ERR_STATE unless the context's reads are those of an elba_set_reads_text call (any other elba_set_reads*, or
 * elba_adopt_trimmed_reads, has replaced them).  elba_get_stat "text_tile_bytes" / "text_scan_span": the tile of the two passes over
 * the chunk and the span of one scan workgroup (constants; tests size inputs from them). */
enum { ELBA_TEXT_AUTO = 0, ELBA_TEXT_FASTA = 1, ELBA_TEXT_FASTQ = 2 };
typedef struct { int32_t format, flags /* 0 */; int64_t first_global_id; } elba_text_cfg;
typedef struct {
    int64_t nreads, bases, packed_bytes, chunk_bytes, lines;
    int32_t format, reserved;     /* format: ELBA_TEXT_FASTA or ELBA_TEXT_FASTQ, as decided */
    float   ms_total;             /* H2D copy of the chunk + index + encode + D2H of the index */
    float   ms_index;             /* count pass .. scan of the byte offsets, the first read-back included */
    float   ms_encode;            /* the encode kernel alone */
} elba_text_stats;
int  elba_set_reads_text(elba_ctx *ctx, const char *chunk, int64_t chunk_bytes, uint64_t chunk_file_offset, const elba_text_cfg *cfg, elba_text_stats *stats);
int  elba_export_read_index(elba_ctx *ctx, elba_fasta_record_t *recs, uint64_t *name_pos, uint32_t *name_len, int64_t nreads_capacity);
/* The resident reads back on the host in DnaBuffer layout: packed[packed_bytes], byte_off[nreads], len[nreads] (caller-allocated;
 * any pointer may be NULL to skip it).  Sizes: elba_ingest_stats, or nreads and sum((len+3)/4). */
int  elba_export_reads(elba_ctx *ctx, uint8_t *packed, int64_t packed_capacity, uint64_t *byte_off, uint32_t *len, int64_t nreads_capacity);
/* What a call invalidates is decided in one table, elba_amd/csrc/state.hpp.  The rule of the matrices: a call that replaces A or B —
 * elba_count_kmers, elba_create_kmer_matrix, elba_set_kmer_matrix[_device], elba_create_seed_matrix, elba_seed_matrix_begin / _send,
 * elba_dist_count_records, elba_dist_set_panel — invalidates B, the alignments of the old B and the pileup, and with them the string graph
 * and its contigs unless the graph was built from an edge list loaded with elba_set_overlaps (or left by elba_prune_reads), which stays
 * loaded.  All but the seed-matrix calls also invalidate A as soon as their arguments are accepted, so one that fails later
 * leaves no A; elba_count_kmers, elba_dist_count_records and elba_set_kmer_matrix[_device] invalidate the k-mer counts as well (the
 * triples land where the counted columns live).  Calls that need what is gone return ELBA_ERR_STATE. */
int  elba_count_kmers(elba_ctx *ctx, elba_kmer_stats *stats);
int  elba_create_kmer_matrix(elba_ctx *ctx, elba_matrix_stats *stats);

/* A as COO triples in any order (duplicates kept: SumDuplicates=false, src/KmerOps.cpp:400). */
int  elba_set_kmer_matrix(elba_ctx *ctx, int64_t nrows, int64_t ncols, int64_t nnz,
                          const int64_t *rows, const int64_t *cols, const uint32_t *vals, elba_matrix_stats *stats);

/* The same with the three arrays resident in HBM (int64 rows, int64 cols, uint32 vals): what a GPU-resident caller of create_seed_matrix(A, AT)
 * (include/SharedSeeds.hpp:98-99) hands over.  elba_export_triples_device writes the resident A back as such triples into
 * caller-allocated device arrays of nnz elements each; their ORDER is unspecified (row-major for most matrices, column-major when the rows
 * carry inline partners, a_csr_format == ELBA_CSR_INLINE: such rows are rebuilt from the columns) — elba_set_kmer_matrix_device takes any order. */
int  elba_set_kmer_matrix_device(elba_ctx *ctx, int64_t nrows, int64_t ncols, int64_t nnz,
                                 const void *d_rows, const void *d_cols, const void *d_vals, elba_matrix_stats *stats);
int  elba_export_triples_device(elba_ctx *ctx, void *d_rows, void *d_cols, void *d_vals);

int  elba_create_seed_matrix(elba_ctx *ctx, elba_overlap_stats *stats);

/* PairwiseAlignment (src/PairwiseAlignment.cpp:5-106) on one rank, on the GPU: x-drop seed-and-extend from seeds[0] of every stored
 * B(i,j), i < j (xdrop_aligner src/XDropAligner.cpp:224-282 with the reference's defaults mat 1, mis -1, gap -1, dropoff 15,
 * src/main.cpp:53-56), classification and Overlap fields.  Needs the reads and B resident on this context (all reads local). */
int  elba_align_seeds(elba_ctx *ctx, int mat, int mis, int gap, int dropoff, elba_align_stats *stats);
/* Multi-GPU: on a row shard of B (after elba_dist_set_panel + elba_create_seed_matrix) elba_align_seeds aligns this rank's share of the
 * candidate pairs — pair {i < j} belongs to the rank of row i when i + j is even, to the rank of row j when it is odd; always as
 * (query i, target j) — once every read of the run is resident: device arrays in DnaBuffer layout with GLOBAL read ids, replicated by
 * the driver with one all-gather (the reads are 2 bits per base). */
int  elba_dist_set_all_reads(elba_ctx *ctx, const void *d_packed, int64_t packed_bytes, const void *d_byte_off, const void *d_len, int64_t nreads_total);
int  elba_export_overlaps(elba_ctx *ctx, elba_overlaps_t *out);
void elba_free_overlaps(elba_overlaps_t *o);

/* The string graph: what src/main.cpp:305-312 does to the R of PairwiseAlignment —
 *   find_bad_reads (src/main.cpp:553-571; reads whose (passed + 1) / (aligned + 1) <= bad_read_cutoff), Prune(!passed), PruneFull(bad),
 *   find_contained_reads (:573-583), PruneFull(contained), TransitiveReduction (src/TransitiveReduction.cpp:3-90; MinPlusSR,
 *   include/TransitiveReduction.hpp:78-110; fuzz = FUZZ, :16, 1000 in the reference).
 * Works on the alignments elba_align_seeds left on this context (one context holding the whole of B), or on an edge list loaded with
 * elba_set_overlaps: host arrays, rows[a] < cols[a] < nreads, strictly ascending in (row, col) — the order elba_export_overlaps gives;
 * a multi-GPU driver concatenates its ranks' shares (merged into that order) and hands them to every rank or to one.
 * elba_export_string_graph returns the entries of S, both triangles, in the order parallel_write_paf walks the reference's S
 * (src/main.cpp:527-541: columns ascending, rows ascending within a column); an entry below the diagonal carries Overlap::Transpose
 * (include/Overlap.hpp:43-69) of its mirror image.  elba_export_read_flags: flags[v] bit 0 = bad read, bit 1 = contained read,
 * bit 2 = removed by elba_clip_tips since, bit 3 = removed by elba_pop_bubbles since, bit 4 = removed by elba_cut_bridges since,
 * bit 5 = removed by elba_resolve_stars since. */
int  elba_set_overlaps(elba_ctx *ctx, int64_t nreads, const int64_t *rows, const int64_t *cols, const elba_overlap_t *vals, int64_t n);
int  elba_transitive_reduction(elba_ctx *ctx, double bad_read_cutoff, int fuzz, elba_string_stats *stats);
int  elba_export_string_graph(elba_ctx *ctx, elba_overlaps_t *out);
int  elba_export_read_flags(elba_ctx *ctx, uint8_t *flags, int64_t nreads);

/* The edge list from HBM, and the pairs a part does not see.
 * elba_set_overlaps_device is elba_set_overlaps with the three arrays on the device (int64 rows, int64 cols, elba_overlap_t vals; n of each):
 * the same conditions, checked by a kernel that finds the smallest offending index, the same ELBA_ERR_INVALID_ARG texts for that index, the
 * same effects on the context.  The arrays are copied device to device: the source may be freed, or be another context's view (the d_rows /
 * d_cols / d_vals of elba_induce_part), and may die afterwards.
 * elba_set_outside_counts[_device] attaches two u32[nreads] arrays to the LOADED edge list (host arrays / device arrays): aligned[v] and
 * passed[v] count pairs of read v that are not in the list — for a part cut out by elba_induce_part, its pairs with a read outside the
 * part.  It needs a valid loaded list (ELBA_ERR_STATE otherwise) of exactly nreads reads and passed[v] <= aligned[v] < 2^31 for every v
 * (ELBA_ERR_INVALID_ARG; the device flavour checks on the device); NULL for both arrays detaches the counts, NULL for one is
 * ELBA_ERR_INVALID_ARG.  From the next elba_transitive_reduction on, read v is bad iff
 *   (passed entries of v in the list + passed[v] + 1) / (entries of v in the list + aligned[v] + 1) <= bad_read_cutoff
 * (in double, as before); nothing else reads the counts, and with none attached every result is bit for bit what it was.  Every call that
 * replaces or invalidates the loaded list detaches them: elba_set_overlaps[_device], elba_prune_reads, elba_align_seeds, a new read set. */
int  elba_set_overlaps_device(elba_ctx *ctx, int64_t nreads, const void *d_rows, const void *d_cols, const void *d_vals, int64_t n);
int  elba_set_outside_counts(elba_ctx *ctx, int64_t nreads, const uint32_t *aligned, const uint32_t *passed);
int  elba_set_outside_counts_device(elba_ctx *ctx, int64_t nreads, const void *d_aligned, const void *d_passed);

/* Contigs: GenerateContigs (src/ContigGeneration.cpp:18-51,110,376-457) on the S of elba_transitive_reduction, one rank.  Reads of degree > 2
 * in S are branches and are dropped; the rest falls into paths, cycles and isolated reads; every path of >= 2 reads is walked from its
 * smaller-id end, and its contig is the concatenation over the chain of the first `prefix` bases of each read (reverse-complemented when the
 * strand bit is set): prefix = suffixT of the walk's S(cur, next), the whole read for the last one.  Contigs come in the reference's emission
 * order (ascending start read).  Cycles emit nothing.  The reads 0 .. nreads-1 of the graph must be on the context: its own reads
 * (elba_set_reads*, as many as the graph has) or the replicated set of elba_dist_set_all_reads; otherwise ELBA_ERR_STATE.  A prefix outside
 * [0, len] (undefined behaviour in the reference) fails with ELBA_ERR_INVALID_ARG and leaves no contigs.  elba_transitive_reduction, every
 * new read set and a replaced A or B under a graph of this context's own alignments invalidate the contigs: the exports and the contig_*
 * counters of elba_get_stat answer only while both the graph and its contigs are valid.  The writer (formats.write_contigs_fasta, hostcpp parallel_write_contigs) writes ">contig<i>\n<seq>\n" per contig (src/main.cpp:496-499). */
typedef struct {
    int64_t nreads, branches, components;   /* components: CC's count on S without the branches' edges, size-1 components included (:51) */
    int64_t used_components;                /* components of >= 2 reads (:110): contigs + cycles */
    int64_t contigs, cycles, contig_reads, bases, longest;   /* contig_reads: chain elements; bases: sum of contig lengths; longest: in bases */
    float   ms_total, ms_rank;              /* device time of the stage / the pointer-jumping rounds */
} elba_contig_stats;

typedef struct {
    int64_t n;                 /* contigs, in the reference's emission order */
    int64_t *seq_off;          /* [n+1] into seq */
    char    *seq;              /* ASCII ACGT, not NUL-separated */
    int64_t *chain_off;        /* [n+1] into the chain arrays */
    int64_t *chain_read;       /* global read id */
    int32_t *chain_prefix;     /* bases taken from that read */
    uint8_t *chain_strand;     /* 1 = reverse complement */
} elba_contigs_t;

int  elba_generate_contigs(elba_ctx *ctx, elba_contig_stats *stats);

/* Two opt-in extensions of elba_generate_contigs; elba_generate_contigs(ctx, st) is elba_generate_contigs_ex with flags 0.  Every contig
 * has a start read, and contigs of all kinds come merged by ascending start read (a path's start is its smaller end).
 *   ELBA_CONTIG_CIRCULAR    a cycle (a component of the branch-free graph whose reads all have two kept neighbours; >= 3 reads) is walked
 *                           from its smallest read s towards the smaller of s's two neighbours, once round.  Every element, the last one
 *                           included, takes prefix = suffixT of S(cur, next) and strand = (direction of S(cur, next) >> 1) & 1; for the last
 *                           one next = s, so the sequence closes on itself and the bases s shares with its predecessor are not written
 *                           twice.  A prefix outside [0, len] fails as on a path, the closing element's included.  Strand consistency
 *                           round the cycle is not checked (the reference checks none on paths either).
 *   ELBA_CONTIG_SINGLETONS  every read in no path and no cycle (no kept neighbour, or a branch) whose flags of elba_export_read_flags are 0
 *                           and whose length is not 0 is a contig of one element (read, len, strand 0).  Reads of a cycle are never
 *                           singletons; without ELBA_CONTIG_CIRCULAR they emit nothing.
 * In the stats contigs, contig_reads, bases and longest cover everything emitted; branches, components, used_components and cycles keep
 * their meaning (cycles: found, emitted or not).  elba_get_stat "contig_circular" / "contig_singletons": the counts of the last call.
 * A null cfg, unknown flag bits or a non-zero reserved word: ELBA_ERR_INVALID_ARG, no contigs left valid.
 * elba_export_contig_kinds: one byte per contig of the last call, 0 path, 1 circular, 2 single read; ELBA_ERR_STATE without valid contigs,
 * ELBA_ERR_INVALID_ARG unless ncontigs is their count. */
enum { ELBA_CONTIG_CIRCULAR = 1, ELBA_CONTIG_SINGLETONS = 2 };
typedef struct { int32_t flags; int32_t reserved[3]; } elba_contig_cfg;
int  elba_generate_contigs_ex(elba_ctx *ctx, const elba_contig_cfg *cfg, elba_contig_stats *stats);
int  elba_export_contig_kinds(elba_ctx *ctx, uint8_t *kind, int64_t ncontigs);
int  elba_export_contigs(elba_ctx *ctx, elba_contigs_t *out);
void elba_free_contigs(elba_contigs_t *c);
int  elba_export_read_contigs(elba_ctx *ctx, int64_t *contig_of_read, int64_t nreads);  /* contig index of every read, -1: in none (without the _ex flags: branch, singleton or cycle) */

/* The assembly graph: the contigs as segments and the edges of S at branch reads as links between segment ends, the records of a GFA
 * (formats.write_gfa, hostcpp write_gfa).  elba_generate_contigs* drops every read of degree > 2 with its edges; this call says which
 * contig ends met at which branch read, in which orientation and with how many bases of overlap.  It is an export: it needs a valid S
 * and valid contigs of it, and the reads the contig call needed (otherwise ELBA_ERR_STATE); it changes neither, invalidates nothing and
 * keeps only scratch and the counts of its last call on the context.
 * Segments are the contigs of the last successful elba_generate_contigs*, indexed as elba_export_contigs orders them.  A read is PLACED
 * when elba_export_read_contigs gives it a contig; a placed read is FIRST in its chain, LAST, or both, and has the strand bit of its
 * chain element; it is AS STORED in its contig when that bit is 0.  deg(x) = entries of column x of S.
 *   step        for reads u < v with an entry in S, the step u -> v is the entry the contig walk reads at u (column u, row v: the
 *               Overlap::Transpose of what is stored there): prefix p(u->v) = its suffixT, direction d = the two low bits of its
 *               direction.  u is left reverse-complemented iff d & 2, v is entered as stored iff d & 1.  The step v -> u is the other half
 *               of the same entry: p(v->u) = its suffix, d' = the low bits of its directionT.
 *   candidate   every pair u < v with an entry in column u of S where deg(u) > 2 or deg(v) > 2.  (Edges between two reads of degree <= 2
 *               lie inside a chain or close a cycle: no links.)
 *   unplaced    a candidate one of whose reads is not placed: counted, not emitted.  After a contig call with both ELBA_CONTIG_* flags on a
 *               graph whose reads with entries are unflagged and not empty there are none.
 *   leaving u   the from-segment is u's contig.  from_rev = 0 when u is last and leaves in the orientation it has in the chain (reversed
 *               iff its strand bit is 1); from_rev = 1 when u is first and leaves in the other orientation.  (A chain of one read is
 *               therefore left reversed iff u is.)
 *   entering v  the to-segment is v's contig.  to_rev = 0 when v is first and is entered in its chain orientation; to_rev = 1 when v is
 *               last and is entered in the other orientation.
 *   twisted     a candidate with both reads placed for which neither line of `leaving` or neither line of `entering` holds: the edge
 *               hangs on the side of the read that is interior to its contig (both overlaps on one end).  Counted, not emitted.
 *   overlap     min(len(u) - p(u->v), len(v) - p(v->u)), clamped to [0, min(bases of the two segments)]; `clamped` counts the links
 *               whose value the clamp changed.  No prefix fails the call.
 *   asymmetric  counts the emitted links whose d' is not d with its two bits exchanged, i.e. whose step v -> u is not the reverse
 *               complement of u -> v.  Aligned graphs have none; loaded edge lists can.
 *   closure     every contig of kind circular gives one record: from = to = the contig, from_rev = to_rev = 0, overlap 0 (the sequence
 *               closes on itself without repeating a base), from_read = to_read = its start read, flags bit 0 set.
 *   order       records ascend in (from_read, to_read); an edge link has from_read = u < to_read = v, a closure from_read = to_read, so
 *               keys are unique and the result does not depend on the order in which reads or columns are visited.  Read ids are those
 *               of chain_read.
 * Stats: segments = contigs; candidates = links (edge links only) + twisted + unplaced; closures; clamped and asymmetric are over the edge
 * links.  elba_get_stat "graph_segments", "graph_candidates", "graph_links", "graph_closures", "graph_twisted", "graph_unplaced",
 * "graph_clamped", "graph_asymmetric": the last call's, 0 while the graph or its contigs are not valid.  Read ids beyond 32 bit:
 * ELBA_ERR_UNSUPPORTED.  Cost: S once (8 + 36 bytes per entry), 8 bytes per read for the table and the scan, 24 bytes per record, one host
 * synchronisation for the output size.  A column of more than 64 entries is worked on by a whole wavefront. */
typedef struct { uint32_t from, to;            /* segment (contig) indices */
                 uint32_t from_read, to_read;  /* the reads of the edge (closure: the start read twice) */
                 int32_t  overlap;             /* bases, the GFA's <overlap>M */
                 uint8_t  from_rev, to_rev;    /* 1 = '-' */
                 uint8_t  flags;               /* bit 0: closure of a circular contig */
                 uint8_t  reserved; } elba_link_t;
typedef struct { int64_t n; elba_link_t *links; } elba_links_t;
typedef struct { int64_t segments, candidates, links, closures, twisted, unplaced, clamped, asymmetric;
                 float   ms_total; int32_t reserved; } elba_graph_stats;
int  elba_export_assembly_links(elba_ctx *ctx, elba_links_t *out, elba_graph_stats *stats);   /* out->n = links + closures */
void elba_free_links(elba_links_t *l);

/* Read placements and contig depth: where every read lies on the assembly and how deep every contig base is covered — what a reads-to-contigs
 * PAF (formats.write_placements_paf, hostcpp write_placements_paf) and a GFA depth tag (write_gfa's depth) are written from.
 * elba_export_contigs places the chain reads only; this call also places, through ONE aligned pair each, the reads the graph lost on the way
 * (contained reads, reads a cleaning call removed, branches, reads whose edges the reduction dropped).  It is an export: it needs a valid S
 * and valid contigs of it, the reads the contig call needed and the pairs the graph was built from (the list of elba_set_overlaps /
 * elba_prune_reads, else the context's own alignments), otherwise ELBA_ERR_STATE; it changes none of them, invalidates nothing — a valid
 * pileup included — and keeps only scratch and the counts of its last call on the context.  Every value is an integer: the result is exact
 * and does not depend on the order in which reads or pairs are visited.
 *   oriented    a read of length l that lies on its contig with strand s has the forward interval [b, e) at the oriented interval [b, e)
 *               when s = 0 and at [l - e, l - b) when s = 1.  ob(b, e) is the begin of that oriented interval.
 *   chain read  element e of contig c holding read r with strand s: kind 1, contig c, start = the sum of the prefixes of the elements of c
 *               before e, strand s, anchor r, score 0.
 *   candidate   a pair a of the graph's input with passed != 0 between a read x that is in no contig, has none of cfg->skip_flags in its
 *               flags of elba_export_read_flags and len(x) > 0, and a chain read y; x may be the pair's Q or its T.  Pairs between two chain
 *               reads or between two reads off every chain are no candidates: a read is placed through a chain read, one level deep.
 *   anchor      of the candidates of x the one with the largest max(score, 0), on a tie the one with the smallest index in the input list.
 *   transform   through its anchor pair x gets kind 2, the contig of y, anchor y, score = the pair's score, strand(x) = strand(y) XOR rc and
 *               start(x) = start(y) + ob_y - ob_x, ob taken of the pair's interval on that read with that read's length and strand
 *               (begT / endT are on T's forward strand also under rc).  start is the contig position of base 0 of x in its contig
 *               orientation: unclipped, not wrapped, it may be negative or beyond the contig.
 *   credit      on a path or single-read contig of L bases a placed read of length l credits [max(start, 0), min(start + l, L)): flag bit 0
 *               (clipped) when that differs from [start, start + l), bit 1 (outside) when it is empty — credited nothing, still reported.
 *               On a circular contig it credits min(l, L) bases from start mod L (the mathematical modulo), clipped when l > L; when that
 *               interval crosses L it is split in two at L and the read gets bit 2 (wrapped).  A circular contig of no bases: outside.
 *   depth       per contig the maximal runs of equal depth of the credited intervals from 0 to its length, in the layout elba_pileup_t
 *               has per read: seg_off[c] .. seg_off[c + 1], seg_start ascending from 0, seg_depth; a contig of no bases has no run.
 *               credited_reads[c] = the reads that credited at least one base of c, credited_bases[c] = the sum of their credited lengths
 *               = the sum over c's runs of length x depth.
 *   the others  kind 0, contig -1, start 0, anchor = the read itself: a read off every chain with a skip bit is `skipped`; else one of
 *               length 0 is `empty`; else one without a candidate is `unanchored`.  chain + anchored + unanchored + skipped + empty = nreads.
 * Read ids (anchor) are those of chain_read.  Stats: candidates = the candidate pairs; clipped, outside and wrapped count placed reads;
 * segments = seg_off[ncontigs]; max_depth; credited_bases = the sum over the contigs.  elba_get_stat "place_chain", "place_anchored",
 * "place_unanchored", "place_skipped", "place_candidates", "place_clipped", "place_outside", "place_wrapped", "place_segments",
 * "place_max_depth": the last call's, 0 while the graph or its contigs are not valid.
 * Errors, after each of which nothing of this call is left valid (*out is zeroed): a null cfg, a non-zero reserved word or a skip_flags
 * outside 0 .. 255 (the flags are one byte): ELBA_ERR_INVALID_ARG.  A candidate whose Q or T interval is outside [0, len] or has beg > end: ELBA_ERR_INVALID_ARG, the message names
 * the smallest such pair (pairs that are no candidates are not looked at).  A contig of 2^31 bases or more, read ids or pairs beyond 32 bit,
 * or 4 x nreads + ncontigs >= 2^32: ELBA_ERR_UNSUPPORTED.
 * Cost: 52 bytes per pair read, one 64-bit atomicMax per candidate, 24 bytes per read written, 8 bytes per endpoint (two or four per
 * crediting read) through the pileup's sort and segment passes, one host synchronisation for the output sizes. */
typedef struct { int32_t skip_flags; int32_t reserved[3]; } elba_place_cfg;   /* reads with any of these bits of elba_export_read_flags are not anchored; 1 (bad reads) is Engine's default */
typedef struct { int64_t start;            /* contig position of base 0 of the read in its contig orientation; unclipped, not wrapped, may be < 0 */
                 int32_t contig;           /* -1: not placed */
                 uint32_t anchor;          /* chain read it was placed through (its own id for a chain read) */
                 int32_t score;            /* the anchor pair's score; 0 for chain reads */
                 uint8_t strand, kind      /* 0 none, 1 chain, 2 anchored */, flags /* bit 0 clipped, 1 outside, 2 wrapped */, reserved; } elba_placement_t;
typedef struct { int64_t nreads, ncontigs; elba_placement_t *reads;
                 int64_t *seg_off; int32_t *seg_start, *seg_depth;   /* per contig: maximal runs of equal depth from 0 to its length, as elba_pileup_t has them per read */
                 int64_t *credited_reads, *credited_bases; } elba_placements_t;
typedef struct { int64_t nreads, chain, anchored, unanchored, skipped, empty, candidates, clipped, outside, wrapped, segments, max_depth, credited_bases; float ms_total; int32_t reserved; } elba_place_stats;
int  elba_place_reads(elba_ctx *ctx, const elba_place_cfg *cfg, elba_placements_t *out, elba_place_stats *stats);
void elba_free_placements(elba_placements_t *p);

/* Contig polishing (not in the reference, which has no consensus step): elba_generate_contigs writes a contig as prefixes of single reads,
 * so every error of a chain read stands in the contig at depth 1 while elba_place_reads puts many other reads on the same bases.  This call
 * aligns every placed read to its stretch of the contig in a band around its placement, lets the alignments vote per contig column and per
 * gap between two columns, and writes the contigs the votes call.  It is an export like elba_place_reads: it needs a valid S, valid contigs
 * of it, the reads and the pairs the graph was built from, otherwise ELBA_ERR_STATE; it changes and invalidates nothing on the context — a
 * valid pileup and the contigs themselves stay as they are — and keeps only scratch and the counts of its last call.  Every value is an
 * integer and every sum is commutative: the result does not depend on the order in which reads, rows or votes are visited.
 *   placement   the records of elba_place_reads under cfg->skip_flags.  The voters are the reads of kind 1 (chain) and kind 2 (anchored)
 *               without flag bit 1 (outside).
 *   slice       r = the voter in contig orientation (its reverse complement when strand = 1), l its length, start its record's start; L the
 *               length of its contig and s the contig's bases.  On a path or single-read contig i0 = max(0, -start), i1 = min(l, L - start);
 *               on a circular contig i0 = 0, i1 = min(l, L).  n = i1 - i0 (>= 1 for a voter), st = start + i0, q = r[i0 .. i1): q[0] is
 *               expected at column st.  A circular contig is used in unrolled coordinates: column j means s[j mod L] with the mathematical
 *               modulo, st may be negative, gaps and columns are reduced mod L only where votes are added.
 *   band        W = cfg->band.  Cell (i, j) exists when 0 <= i <= n and 0 <= j - i - st + W/2 < W, and, on a contig that is not circular,
 *               0 <= j <= L.  D of a cell that does not exist is infinite, and infinity + 1 = infinity.
 *   distance    D[0][j] = 0 (the begin on the contig is free).  For i >= 1, D[i][j] = the minimum of
 *                   D[i-1][j-1] + (q[i-1] != s[j-1])      diagonal
 *                   D[i-1][j] + 1                         up: the read base q[i-1] is inserted in front of column j
 *                   D[i][j-1] + 1                         left: the contig base s[j-1] is deleted
 *               and the cell's choice is the first of diagonal, up, left whose term equals that minimum.  The end cell is the (n, j) with the
 *               smallest D, of several the one with the smallest j (cell (n, st + n) of the main diagonal is finite, so one exists); dist =
 *               its D, end_j its j.  The read is rejected when dist > (cfg->max_diff_q16 * n) >> 16; a rejected read votes nothing.
 *   votes       from the end cell follow the choices until row 0 is reached.  A diagonal step at (i, j) adds 1 to col[j-1][q[i-1]] and goes
 *               to (i-1, j-1); a left step adds 1 to col[j-1][4], the deletion count, and goes to (i, j-1); an up step goes to (i-1, j).  A
 *               maximal run of up steps at one j adds 1 to gap[j][b], b = the base of the run's LAST step, the first in read order: only
 *               one base of an insertion is restored.  Bases are 0 A, 1 C, 2 G, 3 T.  On a circular contig column j-1 and gap j are taken
 *               mod L; a path or single-read contig has the gaps 0 .. L, gap g lying in front of column g.
 *   calls       depth[c] = col[c][0] + .. + col[c][4].  A column with depth[c] < cfg->min_depth keeps its base (a low-depth column).  Any
 *               other column takes the largest of its five counts; equal counts are preferred in the order the contig's own base, A, C, G,
 *               T, deletion; a winning deletion emits nothing (deleted), a winning base other than the contig's own is substituted.  Gap g
 *               emits one base (inserted), the b with the largest gap[g][b], of equal ones the smallest b, when 2 * (gap[g][0] + .. +
 *               gap[g][3]) > span(g); span(g) = min(depth[g-1], depth[g]), on a circular contig with g - 1 taken mod L, on the others
 *               span(0) = depth[0] and span(L) = depth[L-1].  The polished contig: for c = 0 .. L-1 the base of gap c, if any, then the
 *               base of column c, if any; then, where the contig is not circular, the base of gap L.  A contig of no bases stays empty.
 * Output: n contigs in the order of elba_export_contigs, seq_off[n + 1] and seq (ASCII, seq_off[n] bytes); per contig voters (the reads
 * that voted), substituted, deleted, inserted.  With ELBA_POLISH_EXPORT_VOTES in cfg->flags also col_off[n + 1] (the offsets of the
 * UNPOLISHED contigs), col (5 counts per column: contig k's column c at 5 * (col_off[k] + c)), gap (4 counts per gap, every contig having
 * L + 1 slots: contig k's gap g at 4 * (col_off[k] + k + g); slot L of a circular contig stays 0) and one record per read, nreads of them:
 * {dist, n, end_j, status}, status one of ELBA_POLISH_NOT_PLACED (kind 0), _OUTSIDE, _REJECTED, _VOTED; dist and end_j are 0 unless the read
 * was aligned (rejected or voted), n is 0 unless it is a voter.  Without the flag these pointers are null.
 * Stats: nreads; voted + rejected = the voters, outside; low_depth_columns; bases_before / bases_after = the sum of the contig lengths
 * before and after; sum_dist over the reads that voted; cells = the sum of n * W over the voters; batches (below).  elba_get_stat
 * "polish_voted", "polish_rejected", "polish_outside", "polish_low_depth_columns", "polish_bases_before", "polish_bases_after",
 * "polish_sum_dist", "polish_cells", "polish_batches": the last call's, 0 while the graph or its contigs are not valid.
 * The choices of a voter take n * W / 4 bytes until its votes are cast, so the voters are aligned in batches of consecutive reads whose
 * choices fit elba_set_option "polish_trace_bytes" (0, the default: an eighth of the free device memory, at least 64 MiB); a read that alone
 * exceeds it is a batch of its own.  Votes are integer sums: batches do not change the result.
 * Errors, after each of which nothing of this call is left valid (*out is zeroed): a null cfg, a band other than 64, 128 or 256, a
 * max_diff_q16 outside 0 .. 65536, min_depth < 1, flags other than ELBA_POLISH_EXPORT_VOTES, a non-zero reserved word or a skip_flags
 * outside 0 .. 255: ELBA_ERR_INVALID_ARG, as is a candidate pair with a bad interval (elba_place_reads).  What elba_place_reads does not
 * support, a contig of 2^30 bases or more, a placed read of 2^24 bases or more, or 5 x the contig bases + 4 x the contigs at 2^32 or more: ELBA_ERR_UNSUPPORTED.
 * Cost: elba_place_reads' pair pass; per voter n rows of W cells in registers (one wavefront per read, no memory but W / 4 bytes of
 * choices per row written and read once, and 2 bits per read base); one integer atomic per vote; 36 bytes per contig column for the calls,
 * two host synchronisations (the batch plan and the output size). */
enum { ELBA_POLISH_EXPORT_VOTES = 1 };                                                /* elba_polish_cfg.flags */
enum { ELBA_POLISH_NOT_PLACED = 0, ELBA_POLISH_OUTSIDE = 1, ELBA_POLISH_REJECTED = 2, ELBA_POLISH_VOTED = 3 };   /* elba_polish_read_t.status */
typedef struct { int32_t skip_flags, band, max_diff_q16, min_depth, flags; int32_t reserved[3]; } elba_polish_cfg;   /* Engine's defaults: 1, 64, 16384 (0.25), 3, 0 */
typedef struct { int32_t dist, n, end_j, status; } elba_polish_read_t;
typedef struct { int64_t n; int64_t *seq_off; char *seq;
                 int64_t *voters, *substituted, *deleted, *inserted;
                 int64_t nreads; int64_t *col_off; uint32_t *col, *gap; elba_polish_read_t *reads; } elba_polished_t;
typedef struct { int64_t nreads, voted, rejected, outside, low_depth_columns, bases_before, bases_after, sum_dist, cells, batches;
                 float ms_total, ms_align; } elba_polish_stats;
int  elba_polish_contigs(elba_ctx *ctx, const elba_polish_cfg *cfg, elba_polished_t *out, elba_polish_stats *stats);
void elba_free_polished(elba_polished_t *p);

/* Connected components: which reads belong together.  The reference labels the string graph with LACC (GetRead2Contigs,
 * src/ContigGeneration.cpp:51) and deals the components of two or more reads out to its ranks (GetContigSizes, GetLocalProcAssignments:
 * the largest first, each to the rank with the smallest sum so far).  elba_graph_components labels either graph of a context, every read
 * included; elba_partition_components is that dealing made deterministic.  Both are exports: they need the graph they label (otherwise
 * ELBA_ERR_STATE), change no product, invalidate nothing — contigs, links, placements, pileup and trimmed reads stay as they are — and keep
 * only scratch and the counts of the last call on the context.  Every value is an integer: the result is a function of the graph alone and
 * does not depend on the order in which reads or edges are visited or in which atomics arrive.
 *   vertices    ELBA_CC_STRING: the reads 0 .. M-1 of the current S (M = its read count).  ELBA_CC_OVERLAPS: the reads 0 .. M-1 of the
 *               graph's input — the list of elba_set_overlaps / elba_prune_reads while one is valid, else this context's own alignments;
 *               a context that aligned a row shard is refused as everywhere else.
 *   edges       ELBA_CC_STRING: the unordered pairs {u, v}, u != v, with an entry in S at (u, v), at (v, u) or both — each pair once.  (S
 *               holds both triangles, but the reduction drops an image without a direction alone: a pair can have one entry, on
 *               either side of the diagonal.  It is one edge like the others.)  ELBA_CC_OVERLAPS: the pairs of the input with passed != 0 (the reference's
 *               Prune(!passed)) and nothing else: bad and contained reads keep their edges, so that a contained read lies in its
 *               container's component.
 *   component   a maximal set of reads that reach one another over edges.  Every read is in exactly one; a read without an edge is a
 *               component of one read.  Components are numbered 0 .. n-1 by ascending smallest read: comp_of_read[v] = the number of
 *               components whose smallest read is below the smallest read of v's.  first_read[c] = that smallest read + the id base
 *               (the ids elba_export_string_graph / elba_export_overlaps show).
 *   deg(v)      the edges with v at one end.
 *   per component c   reads[c] = its reads; edges[c] = its edges; branches[c] = its reads with deg > 2; ends[c] = its reads with deg = 1;
 *               bases[c] = the sum of its reads' lengths in 64 bits when ELBA_CC_BASES is set (the lengths of the M reads must be on the
 *               context: ELBA_ERR_STATE otherwise), else 0.  branches = 0 and ends = 2: a path; branches = 0, ends = 0, reads >= 3: a
 *               ring; reads = 1: a lone read.
 * Stats: components = n; used_components = those of two or more reads; isolated = those of one; largest_reads / largest_bases = reads and
 * bases of the component with the most reads (the smaller number on a tie); passes = kernel launches that walked the edge list or the
 * label array — it grows with the logarithm of the read count, not with the graph's diameter.  elba_get_stat "cc_components",
 * "cc_used_components", "cc_largest_reads", "cc_passes": the last labelling's, 0 once the graph it labelled is no longer valid.
 * Errors: a null cfg or output, an unknown graph, an unknown flag, a non-zero reserved word: ELBA_ERR_INVALID_ARG.  Read ids beyond 32 bit
 * (M + id base >= 2^32 - 1 or M >= 2^31 - 1): ELBA_ERR_UNSUPPORTED.  More passes than the hard cap: ELBA_ERR_INTERNAL.
 * Cost: 16 bytes per entry of the edge list per pass over it (+ 1 byte of the record of an input pair; for S a binary search in one
 * column per entry above the diagonal), three passes; 4 bytes per read per
 * pass over the labels; one 32-bit compare-and-swap per edge that joins two trees; one host synchronisation per batch of four flattening
 * passes (one batch on every graph seen so far) and one for the tables. */
enum { ELBA_CC_STRING = 0, ELBA_CC_OVERLAPS = 1 };
enum { ELBA_CC_BASES = 1 };                                   /* flags */
typedef struct { int32_t graph, flags, reserved[2]; } elba_cc_cfg;
typedef struct { int64_t nreads, n;
                 int32_t *comp_of_read;                       /* [nreads] */
                 int64_t *first_read, *reads, *bases, *edges, *branches, *ends; /* [n] each */ } elba_components_t;
typedef struct { int64_t nreads, edges, components, used_components, isolated, largest_reads, largest_bases;
                 int32_t passes, reserved; float ms_total, ms_label; } elba_cc_stats;
int  elba_graph_components(elba_ctx *ctx, const elba_cc_cfg *cfg, elba_components_t *out, elba_cc_stats *stats);
void elba_free_components(elba_components_t *c);

/* The reference's greedy assignment of components to parts (src/ContigGeneration.cpp:126, :184-197), with its open ends closed.  The call
 * labels cfg->graph itself (no labels persist between calls, so none can go stale after a cleaning call), then:
 *   weight(c)   reads[c] when cfg->weight = 0, bases[c] when cfg->weight = 1 (which implies ELBA_CC_BASES and its condition).
 *   order       the components with reads[c] >= min_reads, by weight descending, the smaller component number first on a tie.
 *   deal        in that order each component goes to the part whose sum of weights so far is smallest, the lowest part index on a tie
 *               (std::min_element).  part_weight[p] = the sum of part p at the end.
 *   reads       part_of_read[v] = the part of v's component, -1 when that component has fewer than min_reads reads.
 * Guarantee of the rule: max - min of part_weight is at most the largest weight dealt.  nreads must be the graph's read count.
 * Errors: null cfg or arrays, nparts < 1, weight outside {0, 1}, min_reads < 0, a non-zero reserved word, an unknown graph, a wrong nreads:
 * ELBA_ERR_INVALID_ARG; otherwise as elba_graph_components. */
typedef struct { int32_t graph, nparts, weight /* 0 reads, 1 bases */, min_reads /* the reference: 2 */, reserved[4]; } elba_part_cfg;
int  elba_partition_components(elba_ctx *ctx, const elba_part_cfg *cfg, int32_t *part_of_read, int64_t nreads, int64_t *part_weight /* [nparts] */);

/* The induced sub-problem of one part: what the reference's GetInducedReadSequences and ImposeMyReadDistribution (src/ContigGeneration.cpp)
 * do with local_proc_assignments, cut out on the device.  elba_induce_part is an export in the sense of elba_graph_components: it reads the
 * graph's input (M reads; the list of elba_set_overlaps[_device] / elba_prune_reads while one is valid, else this context's own alignments; a
 * context that aligned a row shard: ELBA_ERR_STATE) and, with ELBA_INDUCE_BASES, the bases of those M reads (ELBA_ERR_STATE when they are not
 * on the context), changes no product and invalidates nothing.  Every value is an integer and no result depends on the order of atomics.
 *   selection   read v (0 <= v < M) is selected iff part_of_read[v] == cfg->part.  Any int32 is allowed; part = -1 selects what
 *               elba_partition_components left unassigned.  nreads must be M.
 *   numbering   old_of_new[0 .. reads) = the selected reads ascending: the new numbering preserves the order.  Ids are local to the graph's
 *               input; stats.id_base is what elba_export_overlaps / elba_export_string_graph add to them.
 *   reads       (ELBA_INDUCE_BASES) DnaBuffer layout exactly as elba_trim_reads leaves it: len'[w] = len[old_of_new[w]]; byte_off'[w] = the
 *               running 64-bit sum of (len' + 3) / 4; the bytes are copied; the unused low bits of a read's last byte are zero; 16 zeroed
 *               guard bytes follow the last read (d_packed / packed hold packed_bytes + 16).  Without the flag d_packed, d_byte_off, d_len
 *               (and their host copies) are NULL and packed_bytes is 0.
 *   pairs       pair a of the input is kept iff both of its reads are selected.  The output keeps the input's order — the numbering is
 *               monotone, so it is again strictly ascending in (row, col) —, rows and cols renumbered, vals bit for bit the input's 36 bytes.
 *   outside     outside_aligned[w] = the input pairs with exactly one read selected, that read being old_of_new[w]; outside_passed[w] = those
 *               of them with passed != 0.  stats.split_pairs and stats.split_passed are their sums over w.
 *   empty       no read selected is no error: reads = pairs = packed_bytes = 0, and the result loads as a context of 0 reads.
 * Device views (d_*) stay valid until the next elba_induce_part on this context, elba_release_workspace or elba_ctx_destroy.  With
 * ELBA_INDUCE_HOST the call also returns malloc'ed host copies (elba_free_induced frees them; arrays of 0 elements are still non-NULL), else
 * the host pointers are NULL.  A failed call leaves *out zeroed.
 * Loading a part: elba_set_reads[_device] with the reads, elba_set_overlaps[_device](reads, rows, cols, vals, pairs),
 * elba_set_outside_counts[_device](reads, outside_aligned, outside_passed), on any context.
 * The guarantee.  Let part_of_read come from elba_partition_components with graph = ELBA_CC_OVERLAPS on the same input, any nparts and
 * min_reads.  Every passed pair lies inside one component and so inside one part: split_passed == 0 for every part (and for part -1).  Load
 * a part with its reads, pairs and outside counts and run elba_transitive_reduction with the same cutoff and fuzz.  Then flag bits 0 and 1 of
 * new read w are those of old_of_new[w] in the whole run (deg and pas of the bad-read rule are the whole run's: inside + outside; contained
 * marks, the symmetrised R and the products of the reduction only ever follow passed pairs, which do not leave the part), and the new S is the whole
 * run's S restricted to the part and renumbered, in the same export order.  Every call that reads only S, the flags, the reads and the
 * passed pairs therefore returns the whole run's result restricted to the part: the five cleaning calls, contigs under all four flag
 * combinations, links, placements, polish, and elba_read_pileup with mode = 0.  NOT covered: elba_read_pileup with mode = 1 (score > 0) when
 * split_pairs > 0 — a failed pair with a positive score adds depth in the whole run and is absent from the part.  A selection that splits
 * passed pairs (split_passed > 0) is served and counted but carries no guarantee.  Without the outside counts the guarantee fails as soon
 * as one failed pair leaves the part: a read with 1 passed pair inside and 3 failed pairs outside has (1 + 1) / (4 + 1) <= 0.65 in the
 * whole run and (1 + 1) / (1 + 1) in its part.
 * Errors: null cfg, out or part_of_read, nreads != M, an unknown flag, a non-zero reserved
 * word: ELBA_ERR_INVALID_ARG.  Read ids beyond 32 bit (M + id base >= 2^32 - 1 or M >= 2^31 - 1) or 2^31 - 1 pairs or more:
 * ELBA_ERR_UNSUPPORTED.  elba_get_stat "induce_reads", "induce_pairs", "induce_split_pairs": those of the last call that succeeded.
 * Cost: 4 B of part_of_read per read (copied to the device), 12 B per read read for the lengths and offsets; 16 + 1 B per input pair read by
 * the mark; 52 B read and 52 B written per kept pair; bases / 4 read and written by the gather; one atomic per straddling pair and counter
 * on its read's outside counters; two host synchronisations (the three sizes, then the counters) and one more for the host copies. */
enum { ELBA_INDUCE_BASES = 1, ELBA_INDUCE_HOST = 2 };           /* flags */
typedef struct { int32_t part, flags, reserved[2]; } elba_induce_cfg;
typedef struct {
    int64_t reads, pairs, packed_bytes;
    /* device views */
    const void *d_old_of_new /* i64[reads] */, *d_packed, *d_byte_off /* u64 */, *d_len /* u32 */,
               *d_rows, *d_cols /* i64[pairs] */, *d_vals /* elba_overlap_t[pairs] */,
               *d_outside_aligned, *d_outside_passed /* u32[reads] */;
    /* host copies when ELBA_INDUCE_HOST is set, else NULL */
    int64_t *old_of_new; uint8_t *packed; uint64_t *byte_off; uint32_t *len;
    int64_t *rows, *cols; elba_overlap_t *vals; uint32_t *outside_aligned, *outside_passed;
} elba_induced_t;
typedef struct { int64_t nreads_in, pairs_in, reads, pairs, bases, packed_bytes, split_pairs, split_passed, id_base;
                 float ms_total, ms_pairs, ms_gather; } elba_induce_stats;
int  elba_induce_part(elba_ctx *ctx, const elba_induce_cfg *cfg, const int32_t *part_of_read, int64_t nreads,
                      elba_induced_t *out, elba_induce_stats *stats);
void elba_free_induced(elba_induced_t *o);

/* Tip clipping (not in the reference, whose GenerateContigs drops every read of degree > 2 with its edges: one stray read hanging off a good
 * path cuts it into three contigs and loses the branch read).  elba_clip_tips works on the S of elba_transitive_reduction, in place, between
 * that call and elba_generate_contigs*.  The rule is on degrees alone — no sequence, no suffix, no length in bases — and is stated on the
 * columns of S: deg(v) = entries of column v, the neighbours of v = their rows (S holds both triangles; where the reduction kept only one
 * image of a pair, the direction -1 case, the same statements hold on the columns as they are).  One ROUND, on the degrees as it finds them:
 *   dead end   a read of degree 1.
 *   tip        from a dead end v1 walk v1, v2, ...: v2 is v1's neighbour, and from a read vi (i > 1) of degree 2 the walk goes on to the
 *              neighbour that is not v(i-1) (the smaller one, should neither be).  The first read b of degree >= 3 ends it: v1 .. vt, t <=
 *              max_tip_reads, is a tip of t reads anchored at b.  A read of degree 1 (or 0) ends it too: a plain path, no tip.  A chain that
 *              would take more than max_tip_reads reads is no tip.
 *   sparing    T(b) = tips anchored at b.  T(b) < deg(b): every tip at b is removed.  T(b) >= deg(b) (a star of short chains): none is, and
 *              b counts once as a spared anchor — clipping never erases a whole component.
 *   removal    every entry of S whose row or column is a read of a removed tip goes, in both triangles; the other entries keep their values
 *              and their order (columns ascending, rows ascending within a column).
 * Up to `rounds` rounds run, each on the S the one before left (an anchor that fell to degree 2 joins two chains, one that fell to degree 1
 * is a new dead end); the call stops after a round that removed nothing (rounds_run counts that round).  The result does not depend on the
 * order in which reads are looked at.  A removed read gets bit 2 (value 4) in the flags of elba_export_read_flags until the next
 * elba_transitive_reduction rebuilds them; since ELBA_CONTIG_SINGLETONS emits only reads whose flags are 0, a clipped read does not come
 * back as a contig of its own.
 * After ELBA_OK the context's S is the clipped one (elba_export_string_graph returns it, elba_generate_contigs* walks it), contigs made
 * before are invalid as after elba_transitive_reduction, and a second call clips further from there.  An S without entries or reads: ELBA_OK,
 * nothing removed, rounds_run 1.  ELBA_ERR_STATE without a valid S; ELBA_ERR_INVALID_ARG for a null cfg, a value out of range or a non-zero
 * reserved word: S, the flags and the contigs stay as they were.
 * Stats: tips counts the tips found, removed or spared; tips, reads_removed, entries_removed (both triangles) and spared_anchors are summed
 * over the rounds; ms_compact is the compaction of the first round (keep flags, scan, scatter), the one that moves the whole of S.
 * Cost of `rounds`: rounds are queued four at a time and the host looks at the device counters once per four; a call that is finished within
 * four rounds (or asks for at most four) synchronises once, and whatever `rounds` is, at most three rounds that have nothing to do are queued
 * (each returns at once but for a scan of 4 bytes per entry).  rounds = 64 is a fair way to say "to the end". */
typedef struct { int32_t max_tip_reads;   /* 1 .. 65535 */
                 int32_t rounds;          /* 1 .. 64: at most this many */
                 int32_t reserved[2]; } elba_tip_cfg;
typedef struct { int64_t nreads, nnz_before, nnz_after;
                 int64_t dead_ends;       /* degree-1 reads when round 1 starts */
                 int64_t tips, reads_removed, entries_removed, spared_anchors;  /* summed over the rounds */
                 int32_t rounds_run, reserved;
                 float   ms_total, ms_compact; } elba_tip_stats;
int  elba_clip_tips(elba_ctx *ctx, const elba_tip_cfg *cfg, elba_tip_stats *stats);

/* Bubble popping (not in the reference either).  A bubble is two or more short chains of degree-2 reads between the same two branch reads: a
 * heterozygous site, a run of reads with one systematic error, an overlap the reduction could not prove redundant.  Both end reads have
 * degree 3 and are dropped by elba_generate_contigs*, so one bubble breaks a path into four contigs (before, arm, arm, after), and a cycle
 * into three linear ones.  elba_pop_bubbles works on the S of elba_transitive_reduction, in place, between that call and
 * elba_generate_contigs*, before or after elba_clip_tips.  The rule is stated on the columns of S alone, as the tips rule is: deg(v) = entries of
 * column v, the neighbours of v = their rows; no sequence, no suffix, no direction, no length in bases.  One ROUND, on the degrees as it finds
 * them:
 *   anchor     a read of degree >= 3.
 *   arm        for an anchor a and an entry of column a whose row v1 has degree 2, the tips walk: from a read vi of degree 2 it goes on to the
 *              row of column vi that is not the read it came from (the smaller one, should neither be); for v1, "came from" is a.  The first
 *              read b of degree >= 3 ends it: v1 .. vt, 1 <= t <= max_arm_reads, is an arm of t reads from a to b.  There is no arm if the
 *              walk ends at a read of degree 0 or 1, if it returns to a (b == a), or if it would need more than max_arm_reads reads.  A direct
 *              entry between two anchors is no arm (t >= 1).  Every arm is recorded once, at its smaller anchor (a < b); its first read is the
 *              one in a's column.
 *   bubble     the set of all arms with the same (a, b), when there are two or more.
 *   kept arm   the arm with the most reads; on a tie the one whose first read is smallest (the earliest entry of column a).  Every other arm
 *              of the bubble is removed.  A direct entry a - b stays.  (After the reduction an arm is a minimal chain over its span, so more
 *              reads mean more coverage; overlap scores, lengths in bases and strands are not looked at.)
 *   removal    every entry of S whose row or column is a read of a removed arm goes, in both triangles; the other entries keep their values
 *              and their order (columns ascending, rows ascending within a column).
 * On a symmetric S the arms are disjoint (their reads have degree 2), each belongs to one (a, b), and a bubble keeps one arm: no anchor loses
 * its last edge and no component is erased.  Everything a round decides is read from tables frozen at its start, and what it writes are sets
 * and sums: the result does not depend on the order in which entries are looked at.  Where the reduction kept only one image of a pair (the
 * direction -1 case) the contract is what the statements above produce on the columns as they are; the guarantees are not claimed there.
 * Up to `rounds` rounds run, each on the S the one before left (an anchor that fell to degree 2 joins two chains, so the outer bubble of a
 * nested pair shows one round later); the call stops after a round that removed nothing (rounds_run counts that round).  A removed read gets
 * bit 3 (value 8) in the flags of elba_export_read_flags until the next elba_transitive_reduction rebuilds them, so ELBA_CONTIG_SINGLETONS
 * does not bring it back.
 * Errors and state are those of elba_clip_tips: after ELBA_OK the context's S is the popped one, contigs made before are invalid, and a second
 * call — or elba_clip_tips — goes on from there.  An S without entries or reads: ELBA_OK, nothing removed, rounds_run 1.  ELBA_ERR_STATE
 * without a valid S; ELBA_ERR_INVALID_ARG for a null cfg, a value out of range or a non-zero reserved word: S, the flags and the contigs stay
 * as they were.
 * This call alone does not reach the fixed point of both: a tip on an arm gives the arm a read of degree 3, so there is no arm until the tip
 * is clipped.  Clip first, then pop, and alternate until both remove nothing (Engine.simplify_graph in the Python binding does).  On a
 * symmetric S a pop makes no new tip — it lowers anchors to degree 2, which only lengthens dead-end chains — so the second pass finds nothing.
 * Stats: arms counts the arms found, in a bubble or not; arms, bubbles, arms_removed, reads_removed and entries_removed (both triangles) are
 * summed over the rounds; ms_compact is the compaction of the first round, as for tips, and `rounds` costs what it costs there: four rounds
 * are queued per look at the device counters.  Picking the kept arm costs, per arm, one pass over its anchor's column. */
typedef struct { int32_t max_arm_reads;   /* 1 .. 65535 */
                 int32_t rounds;          /* 1 .. 64: at most this many */
                 int32_t reserved[2]; } elba_bubble_cfg;
typedef struct { int64_t nreads, nnz_before, nnz_after;
                 int64_t anchors;         /* reads of degree >= 3 when round 1 starts */
                 int64_t arms, bubbles, arms_removed, reads_removed, entries_removed;  /* summed over the rounds */
                 int32_t rounds_run, reserved;
                 float   ms_total, ms_compact; } elba_bubble_stats;
int  elba_pop_bubbles(elba_ctx *ctx, const elba_bubble_cfg *cfg, elba_bubble_stats *stats);

/* Cutting weak overlaps (not in the reference either; the third step of miniasm's cleaning, and at ratio 1 the "best overlap graph").  One
 * kind of branch is left by the two calls above: an end of a read has its true overlap and one or more much weaker ones, from a repeat copy
 * or a chance alignment.  Both lead into long paths (no tip) that do not rejoin within a few reads (no bubble), the read has degree 3 and
 * elba_generate_contigs* cuts the path there.  elba_cut_weak_overlaps works on the S of elba_transitive_reduction, in place, between that call
 * and elba_generate_contigs*, before or after the other two.  It removes ENTRIES, no reads.  The rule is stated on the columns of S as they
 * are.  For an entry z of column c with row r and value o (o = S(r, c), query r, target c; a lower-triangle entry carries Overlap::Transpose
 * of its mirror image):
 *   side(z)    o.direction & 1: the end of read c the overlap lies on (h of Overlap::arrows).  Two entries of one column can be walked
 *              through only if their sides differ (MinPlusSR::multiply refuses t2 == h1).  Every entry of S has a direction of 0 .. 3.
 *   weight(z)  o.score: the one field Overlap::Transpose copies unchanged, so both images of a pair carry the same weight.  It grows with
 *              overlap length and with identity; it is not the length in bases.
 * ONE pass, on tables frozen at its start:
 *   1. for every read c and side e: cnt(c, e) = entries of column c with that side, best(c, e) = their largest score.
 *   2. z is weak at its column when cnt(c, side(z)) >= 2 and best(c, side(z)) > 0 and
 *          (int64) score * 65536 < (int64) min_ratio_q16 * best(c, side(z))
 *      in integer arithmetic, exactly as written.  An entry that ties the best of its side is never weak.
 *   3. z is removed when it is weak at its column, or when its mirror image — the entry of column r whose row is c — is weak at column r.
 *      Where S holds only one image of a pair (the direction -1 case of the reduction), only the first condition applies.
 *   4. survivors keep their values and their order (columns ascending, rows ascending within a column).  No read is removed and the flags
 *      of elba_export_read_flags are untouched.
 * There is no sparing: a read end whose best overlap is weak at the other read loses it and becomes a dead end, which elba_clip_tips then
 * judges (miniasm's behaviour); sides_emptied counts how often that happened.
 * There is no `rounds`: the pass is its own fixed point.  Every survivor of a side had score * 65536 >= ratio * best_old >= ratio * best_new
 * (a side's best and count only fall or stay, and a side whose best was <= 0 had nothing weak), so a second call with the same ratio removes
 * nothing.  And a smaller ratio removes a subset of what a larger one removes: weak at ratio q is weak at every ratio above q.
 * Errors and state are those of elba_clip_tips, row for row: ELBA_ERR_STATE without a valid S; ELBA_ERR_INVALID_ARG for a null cfg, a ratio
 * outside 1 .. 65536 or a non-zero reserved word; both leave S, the flags and the contigs as they were.  An S without entries or reads:
 * ELBA_OK, nothing removed.  After ELBA_OK the context's S is the cut one, contigs made before are invalid, and elba_clip_tips and
 * elba_pop_bubbles go on from there.
 * Stats: counts of the one pass; entries_removed counts both images of a pair; ms_compact spans the keep flags (which here look up every
 * entry's mirror image), the scan and the scatter.  One host synchronisation per call; cost is linear in nnz whatever a column's length. */
typedef struct { int32_t min_ratio_q16;   /* 1 .. 65536: 65536 keeps only entries tied with the best of their side */
                 int32_t reserved[3]; } elba_weak_cfg;
typedef struct { int64_t nreads, nnz_before, nnz_after;
                 int64_t branch_sides;     /* (read, side) with cnt >= 2 before the cut */
                 int64_t weak_entries;     /* entries weak at their own column */
                 int64_t entries_removed;  /* both images */
                 int64_t sides_emptied;    /* (read, side) with cnt >= 1 before and no entry after */
                 float ms_total, ms_compact; } elba_weak_stats;
int  elba_cut_weak_overlaps(elba_ctx *ctx, const elba_weak_cfg *cfg, elba_weak_stats *stats);

/* Cutting bridges (the rule of the reference's asmtools/bridge_removal.py, which runs on a written-out graph after the program; taken here
 * from one read to a chain of reads).  A bridge is a read, or a short chain of reads, that joins the middles of two otherwise independent
 * long paths — a chimeric read that survived the pileup, a repeat copy two loci share — so that the graph looks like the letter H.  Each end
 * read of the bridge has degree 3 and elba_generate_contigs* drops it: an H costs four contigs and three or more lost reads where there are
 * two paths.  Both flanks are long (no tip), the chains do not rejoin (no bubble) and the scores can tie (no weak overlap).
 * elba_cut_bridges works on the S of elba_transitive_reduction, in place, between that call and elba_generate_contigs*, before or after the
 * other three cleaning calls.  The rule is stated on the columns of S alone, as the tips and bubbles rules are: deg(v) = entries of column v,
 * the neighbours of v = their rows; no sequence, no suffix, no score, no direction, no length in bases.  ONE pass, on tables frozen at its
 * start:
 *   anchor     a read of degree >= 3.
 *   chain      exactly the arm of elba_pop_bubbles: for an anchor a and an entry of column a whose row v1 has degree 2, the tips walk: "came
 *              from" is a for v1, and from a read of degree 2 the walk goes on to the first row of its column that is not the read it came
 *              from.  The first read b of degree >= 3 ends it: v1 .. vt, 1 <= t <= max_bridge_reads, is a chain from a to b.  There is no
 *              chain if the walk ends at a read of degree 0 or 1, if b == a, or if it would need more than max_bridge_reads reads.  Every
 *              chain is recorded once, at its smaller anchor (a < b).
 *   flank      for a read u of degree exactly 3 and an entry of column u with row w: walk from w, "came from" u, and count the reads of
 *              degree 2 passed; stop at the first read whose degree is not 2, or when min_flank_reads have been counted.  The flank is LONG
 *              when the count reached min_flank_reads.  A flank that ends in a dead end counts its degree-2 reads only: min_flank_reads - 1
 *              reads of degree 2 followed by a read of degree 1 is short.  (The walk does not ask where it is: round a loop of degree-2 reads
 *              that returns to u it counts the loop's reads once, and in a component that is one cycle it would go round until the count is
 *              reached — but such a component has no anchor to start from.)
 *   bridge     a chain from a to b for which all three hold: deg(a) == 3 and deg(b) == 3; the two entries of column a other than v1's are
 *              both long flanks; column b holds an entry whose row is vt, and its two other entries are both long flanks.  (On a symmetric
 *              S column b always holds vt.)
 *   removal    every read of a bridge gets bit 4 (value 16) in the flags of elba_export_read_flags until the next
 *              elba_transitive_reduction rebuilds them; every entry of S whose row or column is such a read goes, in both triangles; the
 *              other entries keep their values and their order (columns ascending, rows ascending within a column).  a and b stay: each
 *              falls to degree 2, and its two flanks become one path.
 * min_flank_reads > max_bridge_reads is required.  On a symmetric S this gives:
 *   1. A chain is never a long flank: seen from either anchor as a flank it counts t <= max_bridge_reads < min_flank_reads reads and ends
 *      at a read of degree >= 3.  A bridge at a needs the two other entries of column a to be long flanks, so of the three entries of
 *      column a at most one starts a bridge: an anchor has at most one bridge, bridges are disjoint (their reads have degree 2 and lie on
 *      one chain), and no read loses an entry except the bridge's reads, which lose all, and its two anchors, which lose one each.
 *   2. No component is erased: the bridge's reads go, but each anchor keeps two long flanks, 2 * min_flank_reads reads or more.
 *   3. The pass is its own fixed point, so there is no `rounds`.  A chain left uncut between anchors of degree 3 had a short flank: one
 *      that ended, after fewer than min_flank_reads reads of degree 2, at a read x of degree != 2.  After the pass the degree of x is
 *      another only if x is a cut anchor (guarantee 1), reached here through one of its own flanks.  But then the same reads walked the
 *      other way, from x, were a flank of x of fewer than min_flank_reads reads that ended at an anchor: a short flank of x, so x was not
 *      cut.  A chain whose anchor has degree >= 4 keeps it (such an anchor is no bridge's end), and new chains do not appear: a cut anchor
 *      has degree 2 afterwards and only lengthens what passes through it.  A second call with the same cfg removes nothing.
 *   4. With max_bridge_reads = 1 and min_flank_reads = walklen >= 2 the removed entries are those asmtools/bridge_removal.py removes from
 *      the same graph: a read of degree 2 whose two neighbours both have degree 3, each with exactly two walks of at least walklen reads
 *      of degree 2 (that script's third walk, the one through the bridge read, has length 1 and never counts).
 * Where the reduction kept only one image of a pair (the direction -1 case) the contract is what the statements above produce on the
 * columns as they are; the guarantees are not claimed there.
 * Errors and state are those of elba_clip_tips, row for row: ELBA_ERR_STATE without a valid S; ELBA_ERR_INVALID_ARG for a null cfg, a value
 * out of range, min_flank_reads <= max_bridge_reads or a non-zero reserved word; all of these leave S, the flags and the contigs as they
 * were.  An S without entries or reads: ELBA_OK, nothing removed.  After ELBA_OK the context's S is the cut one, contigs made before are
 * invalid, and the other cleaning calls go on from there.  Since ELBA_CONTIG_SINGLETONS emits only reads whose flags are 0, a bridge read
 * does not come back as a contig of its own.
 * Stats: counts of the one pass; entries_removed counts both triangles; ms_compact spans the keep flags, the scan and the scatter.  One host
 * synchronisation per call; an entry of a degree-3 column costs at most min_flank_reads dependent steps, an entry of an anchor's column at
 * most max_bridge_reads more. */
typedef struct { int32_t max_bridge_reads;   /* 1 .. 65534 */
                 int32_t min_flank_reads;    /* max_bridge_reads + 1 .. 65535 */
                 int32_t reserved[2]; } elba_bridge_cfg;
typedef struct { int64_t nreads, nnz_before, nnz_after;
                 int64_t anchors;        /* reads of degree >= 3 */
                 int64_t chains;         /* chains found, cut or not: equals elba_pop_bubbles' `arms` of one round with max_arm_reads = max_bridge_reads on the same S */
                 int64_t long_flanks;    /* entries of degree-3 columns whose flank is long */
                 int64_t bridges, reads_removed, entries_removed;   /* entries: both triangles */
                 float ms_total, ms_compact; } elba_bridge_stats;
int  elba_cut_bridges(elba_ctx *ctx, const elba_bridge_cfg *cfg, elba_bridge_stats *stats);

/* Resolving three-armed stars (the rule of the reference's asmtools/star_resolution.py, which runs on the written-out string graph and
 * overlap graph after the program).  A star is a read u of degree 3 whose three neighbours all have degree 2.  elba_generate_contigs* drops
 * u with its edges, so one spurious overlap at u — typically a repeat copy u shares with a read from elsewhere — costs three contigs and a
 * lost read where there is one path and a stray read.  None of the three arms has to end within max_tip_reads (no tip), the arms need not
 * rejoin (no bubble), u has no second anchor opposite it (no bridge), and the three scores can tie (no weak overlap).  The graph alone
 * cannot say which arm is the stray one; the overlap matrix before the reduction can.  The two true neighbours of u on its path overlap
 * each other: their pair was in R and was removed as transitive through u.  The stray read overlaps neither.
 * elba_resolve_stars works on the S of elba_transitive_reduction, in place, between that call and elba_generate_contigs*, before or after
 * the other four cleaning calls, and beside S it reads the R of that same reduction, which the context keeps on the device and never
 * changes (elba_release_workspace does not free it).  The rule is on the columns of S and on membership in R alone: deg(v) = entries of
 * column v, the neighbours of v = their rows; no sequence, no suffix, no score, no direction, no length.  One ROUND, on tables frozen at
 * its start:
 *   centre     a read u with deg(u) == 3 whose three rows x1 < x2 < x3 each have degree exactly 2.
 *   pair in R  {x, y} is a pair in R when the symmetrised R of the elba_transitive_reduction call that made this S has an entry (row x,
 *              column y).  R is symmetric by construction, so either row answers (the kernel searches the shorter one).  R holds every
 *              input pair that passed and touches no bad and no contained read — the pairs the reduction marked transitive among them,
 *              and the pairs without a direction, which never reach S.
 *   odd arm    let e be how many of {x1,x2}, {x1,x3}, {x2,x3} are pairs in R.  When e == 1 the neighbour in no such pair is the centre's
 *              odd arm w.  When e is 0, 2 or 3 the centre is left alone.
 *   removal    every odd arm gets bit 5 (value 32) in the flags of elba_export_read_flags until the next elba_transitive_reduction
 *              rebuilds them; every entry of S whose row or column is an odd arm goes, in both triangles; the other entries keep their
 *              values and their order (columns ascending, rows ascending within a column).  u stays and falls to degree 2 (lower if
 *              another centre names one of its other neighbours); w's other neighbour loses an entry too.  That is what the script does:
 *              it deletes every edge from and to the star vertex.
 * Up to `rounds` rounds run, each on the S the one before left; the call stops after a round that removed nothing, and rounds_run counts
 * that round, as in elba_clip_tips.  Rounds are needed because one pass is not its own fixed point: a removal can lower a degree-3
 * neighbour of some degree-3 read to degree 2, and that read is then a new centre.  R is never changed; look-ups between reads that an
 * earlier round or an earlier cleaning call removed never occur, because such reads are in no column and no row of S any more.
 * What follows from the statements:
 *   1. The result does not depend on the order in which reads are looked at.  Whether u is a centre, its e and its odd arm are functions
 *      of the round's columns and of R, both frozen; what a round writes is a SET of odd arms, and a read named by two centres is in the
 *      set once: it is flagged once, counted once in reads_removed, and its entries leave once.
 *   2. Only reads of degree 2 are removed: an odd arm is a row of a centre's column, and all three of those have degree exactly 2 on the
 *      tables the round decides on.  So a centre is never removed in the round in which it is a centre.
 *   3. reads_removed <= resolved (= pairs1), with equality unless two centres of one round name the same arm: every centre with e == 1
 *      names exactly one arm, and every removed read was named by at least one.
 *   4. A round that removes nothing is a fixed point of the call: the next round would find the same columns and the same R, hence the
 *      same centres, the same e, and again no arm.  So a further call with any `rounds` removes nothing either, until another call
 *      changes S.
 *   5. Correspondence with the script: with rounds = 1 the removed entries are those asmtools/star_resolution.py deletes from the same S
 *      and R, when both graphs carry both arcs of every edge.  Its stars are the vertices of in-degree 3 whose successors all have
 *      in-degree 2: the centres.  Its `len(star_arcs) == 2` then counts ONE pair among the three neighbours, present as two arcs: e == 1;
 *      its `assert len(tmp) == 1` holds only under that reading (with two distinct pairs the three neighbours are all arc ends and tmp is
 *      empty).  tmp's one vertex is the neighbour in no pair, and the script deletes every edge from and to it.  igraph is not available
 *      to the tests, so the correspondence is by reading, as for asmtools/bridge_removal.py; no fixture was recorded from the script.  (The script runs one pass; its own loop to a fixed point is commented out.  `rounds` is that loop.)
 * Where the reduction kept only one image of a pair (the direction -1 case) the contract is what the statements above produce on the
 * columns as they are; guarantees 2 to 5 are not claimed there (a column can hold a row whose own column does not hold it back, so "u
 * falls to degree 2" and the script's arcs need not hold).  Guarantee 1 holds always.
 * Errors and state are those of elba_clip_tips, row for row: ELBA_ERR_STATE without a valid S; ELBA_ERR_INVALID_ARG for a null cfg, rounds
 * outside 1 .. 64 or a non-zero reserved word; all of these leave S, the flags and the contigs as they were.  An S without entries or
 * reads: ELBA_OK, nothing removed, rounds_run 1.  Index ranges beyond 32 bit: ELBA_ERR_UNSUPPORTED.  After ELBA_OK the context's S is the
 * resolved one, contigs made before are invalid, and the other cleaning calls go on from there.  Since ELBA_CONTIG_SINGLETONS emits only
 * reads whose flags are 0, an odd arm does not come back as a contig of its own.
 * Stats: centres, pairs0 .. pairs3 (centres by e; pairs1 is `resolved`), reads_removed and entries_removed (both triangles) are summed over
 * the rounds — a centre left alone in three rounds counts three times; ms_compact is the compaction of the first round.  Cost of `rounds`: as
 * for elba_clip_tips, one host synchronisation per four rounds.  A read of degree 3 costs three more pointer pairs, a centre three binary
 * searches of at most floor(log2(len)) + 1 dependent 4-byte loads each, len the shorter of the two rows of R. */
typedef struct { int32_t rounds;          /* 1 .. 64: at most this many */
                 int32_t reserved[3]; } elba_star_cfg;
typedef struct { int64_t nreads, nnz_before, nnz_after;
                 int64_t centres, pairs0, pairs1, pairs2, pairs3;      /* summed over the rounds: centres, and centres by e; pairs1 = resolved */
                 int64_t reads_removed, entries_removed;               /* summed over the rounds; entries: both triangles */
                 int32_t rounds_run, reserved;
                 float   ms_total, ms_compact; } elba_star_stats;
int  elba_resolve_stars(elba_ctx *ctx, const elba_star_cfg *cfg, elba_star_stats *stats);

/* Read pileups and chimera flags: PileupVector / GetReadPileup / GetTrimmedInterval (src/PruneChimeras.cpp:14-69,108-158,
 * include/PruneChimeras.hpp), which src/main.cpp never calls, and R->PruneFull(x, x) of the reads it flags.  Runs after elba_align_seeds,
 * before elba_transitive_reduction, on the pairs that call would read: the list of elba_set_overlaps if one is loaded, else this context's
 * alignments (a row shard's fail with ELBA_ERR_STATE).  The lengths of reads 0 .. nreads-1 must be on the context (its own reads or the
 * replicated set of elba_dist_set_all_reads), otherwise ELBA_ERR_STATE.
 *   pileup     every accepted pair (mode 0: passed; mode 1: score > 0) adds 1 on [begQ + margin, endQ - margin) of read Q and on
 *              [begT + margin, endT - margin) of read T; an interval left empty is dropped.  begT / endT are on T's forward strand also when
 *              rc is set (xdrop_aligner maps them back, src/XDropAligner.cpp:275-276; align.hip does the same, and on rc pairs of the tests the
 *              T interval's reverse complement aligns to the Q interval).  An interval outside [0, len] or with beg > end in a credited pair
 *              fails with ELBA_ERR_INVALID_ARG (the reference asserts, :26).
 *   profile    per read, maximal runs of equal depth as (start, depth) segments: starts strictly increasing from 0, neighbours of different
 *              depth, the last one ends at len; a read without intervals is (0, 0), a read of length 0 has none.
 *   trimmed    GetTrimmedInterval's rule with threshold min_depth and the starting maxlen trim_len (2500 in the reference, :36): the run of
 *              depth >= min_depth replaces the best at a base when span > maxlen && curavg > bestavg (curavg in double, as written);
 *              returned half-open [beststart, bestend + 1), or (-1, -1).
 *   flags      bit 0: no run of depth >= min_depth at least min_run long (unsupported); bit 1: two or more (split: chimera candidate).
 * Two deliberate deviations from the reference: both reads of a pair are credited (GetReadPileup credits only the column read of the
 * upper-triangular R, :137-146), and the trimmed interval is the best run (the reference returns the run still open at the last base, :68).
 * elba_prune_reads removes every pair with either end in {v : flags[v] & mask} and loads the kept pairs, in (row, col) order, as the edge
 * list elba_transitive_reduction reads next (elba_export_overlaps still returns the alignments).  A new read set, a replaced A or B, new alignments,
 * elba_set_overlaps and elba_prune_reads invalidate the pileup (ELBA_ERR_STATE on export). */
typedef struct {
    int32_t mode;               /* 0: pairs with passed; 1: every pair with score > 0 */
    int32_t margin;             /* >= 0: bases dropped at each end of every interval */
    int32_t min_depth;          /* >= 1: the threshold */
    int32_t min_run;            /* >= 1: the length of a long run (flags) */
    int32_t trim_len;           /* >= 0: GetTrimmedInterval's starting maxlen */
    int32_t reserved;           /* 0 */
} elba_pileup_cfg;

typedef struct {
    int64_t nreads, pairs, intervals, segments, max_depth;   /* pairs: accepted by the mode; intervals: credited (non-empty after the margin) */
    int64_t unsupported, split, trimmed;                      /* reads with flag bit 0 / bit 1 / a trimmed interval other than [0, len) */
    int64_t trimmed_bases;                                    /* bases inside trimmed intervals */
    float   ms_total;                                         /* device time of the stage */
    float   reserved;
} elba_pileup_stats;

typedef struct {
    int64_t n, nseg;           /* reads, segments */
    int64_t *seg_off;          /* [n+1] into the segment arrays */
    int32_t *seg_start, *seg_depth;
    int32_t *trim_beg, *trim_end;   /* [n] half-open trimmed interval, -1 / -1: none */
    uint8_t *flags;            /* [n] bit 0 unsupported, bit 1 split */
} elba_pileup_t;

int  elba_read_pileup(elba_ctx *ctx, const elba_pileup_cfg *cfg, elba_pileup_stats *stats);
int  elba_export_pileup(elba_ctx *ctx, elba_pileup_t *out);
void elba_free_pileup(elba_pileup_t *p);
int  elba_prune_reads(elba_ctx *ctx, int mask, int64_t *kept);

/* Reads cut to their supported intervals, chimeras split: what GetTrimmedInterval's [beststart, bestend] is computed for (the reference
 * never cuts: src/main.cpp does not call src/PruneChimeras.cpp).  elba_trim_reads turns the intervals of the LAST elba_read_pileup into a
 * new read set on the device, which elba_adopt_trimmed_reads makes the context's own: reads -> pileup -> pieces -> k-mers -> ... -> contigs.
 *   mode 0     one piece per read: its trimmed interval [trim_beg, trim_end); a read with (-1, -1) gives none.
 *   mode 1     one piece per LONG RUN of the read: a maximal run of depth >= min_depth at least min_run bases long, with the min_depth /
 *              min_run of the elba_read_pileup call that made the pileup (the runs the flags count): flag bit 0 <=> no piece, flag bit 1
 *              <=> two or more (while min_len <= min_run).
 * In both modes a piece shorter than min_len (>= 1) is dropped.  Pieces are numbered by (src_read, src_beg) ascending; piece p is bases
 * [src_beg, src_end) of read src_read.  The new set is in DnaBuffer layout, as elba_set_reads_fasta leaves it: byte_off[p] (u64) is the
 * running sum of (len + 3) / 4, len is u32, 16 zeroed guard bytes follow the last piece, and the unused low bits of a piece's last byte
 * are zero whatever follows in the source (DnaSeq::compress, src/DnaSeq.cpp:17).
 * Needs a valid pileup and the bases of its reads on the context (its own reads, as many as the pileup has, or the replicated set of
 * elba_dist_set_all_reads: the choice elba_read_pileup makes for the lengths), otherwise ELBA_ERR_STATE.  A mode other than 0 / 1,
 * min_len < 1 or a non-zero reserved word: ELBA_ERR_INVALID_ARG.
 * The result is a snapshot in buffers of its own: it survives elba_prune_reads and elba_release_workspace; a new read set
 * (elba_set_reads*, elba_dist_set_all_reads), a new elba_read_pileup or a new elba_trim_reads invalidates it (export, get and adopt then
 * return ELBA_ERR_STATE).  Every read dropped is no error: n = 0, packed_bytes = 0, and adopting leaves a context with 0 reads.
 * elba_adopt_trimmed_reads consumes the snapshot: the pieces become the context's reads exactly as after elba_set_reads (first_global_id
 * 0; k-mers, A, B, alignments, edge list, string graph, pileup of the old reads invalidated; elba_export_reads returns the pieces); a
 * second adopt without a new trim is ELBA_ERR_STATE.  The pointers of elba_get_trimmed_reads_device stay valid until the next
 * elba_trim_reads, adopt or destroy. */
typedef struct { int32_t mode; int32_t min_len; int32_t reserved[2]; } elba_trim_cfg;

typedef struct {
    int64_t nreads_in, pieces;                            /* reads of the pileup; pieces written */
    int64_t reads_dropped, reads_split, reads_unchanged;  /* reads with no piece (reads of length 0 included) / two or more / one piece that is [0, len) */
    int64_t bases_in, bases_out, packed_bytes, longest;   /* bases of the reads / of the pieces; bytes of the new packed buffer; longest piece in bases */
    float   ms_total, ms_repack;                          /* device time of the stage / of the repack kernel */
} elba_trim_stats;

typedef struct { int64_t n; int64_t *src_read; int32_t *src_beg, *src_end; } elba_trim_map_t;   /* piece p = bases [src_beg, src_end) of read src_read */

int  elba_trim_reads(elba_ctx *ctx, const elba_trim_cfg *cfg, elba_trim_stats *stats);
int  elba_export_trim_map(elba_ctx *ctx, elba_trim_map_t *out);
void elba_free_trim_map(elba_trim_map_t *m);
int  elba_get_trimmed_reads_device(elba_ctx *ctx, const void **d_packed, int64_t *packed_bytes, const void **d_byte_off, const void **d_len, int64_t *n);
int  elba_adopt_trimmed_reads(elba_ctx *ctx);

int  elba_export_dcsc(elba_ctx *ctx, int64_t row_lo, int64_t row_hi, int64_t col_lo, int64_t col_hi, elba_dcsc_t *out);
void elba_free_dcsc(elba_dcsc_t *d);
int  elba_export_csr(elba_ctx *ctx, int64_t row_lo, int64_t row_hi, elba_csr_t *out);
void elba_free_csr(elba_csr_t *c);
int  elba_export_kmer_matrix(elba_ctx *ctx, elba_kmer_matrix_t *out);
void elba_free_kmer_matrix(elba_kmer_matrix_t *m);
/* histogram of column counts: hist[c] = #reliable k-mers occurring c times, c in [0, upper] (src/main.cpp:449-485) */
int  elba_kmer_histogram(elba_ctx *ctx, int64_t *hist, int64_t len);

int  elba_get_device_view(elba_ctx *ctx, elba_device_view *view);

/* Run-time options by name (unknown name: ELBA_ERR_INVALID_ARG).  Besides the one below: tuning and A/B switches that never change a
 * result (struct Options in elba_amd/csrc/common.hpp lists them: "no_symmetry", "no_ell", "no_pay", "mir32", "no_hints", "no_sample",
 * "no_suffix", "no_row_order", "dense_up", "dense_wgs", "panel_inline", "kmer_pairs", "kmer_unfused", "kmer_no_msd", "csr_pairs", "emit_plain",
 * "trace", "kmer_drop", "dk", "aln_tiers", ...).
 * Options that shape A must be set before elba_count_kmers / elba_set_kmer_matrix.
 *   "overlap_cold_calls" (0 | 1): 1 = every elba_create_seed_matrix call forgets what earlier calls on the same matrix learned (the
 *       distinct-partner ratio that picks the starting table tiers, which tiers and column sorts received rows): what a caller that
 *       multiplies every matrix once pays — the reference's create_seed_matrix is called once per A (src/main.cpp:281).  Buffers stay
 *       allocated.  Default 0.
 *   "kmer_batch_instances" (>= 0): LIMITS.  The reference batches its k-mer exchange so that the input's size is no limit
 *       (include/KmerOps.hpp:10-12,33-56).  Here a context counts any number of k-mer instances for 9 <= k <= 95 — more than this option allows at
 *       once (0, the default: 0xE0000000, what a 32-bit place holds) are counted in PASSES over ranges of the k-mer value (consecutive first
 *       digits of the value partition — 19 <= k <= 31: of its coarse digit, the leading 10 bits of the flattened value, each pass partitioned
 *       finer inside its own range; k > 31: ranges of the leading 24 bits of the first word —: the passes yield consecutive k-mer ids and
 *       consecutive stretches of the columns; every pass enumerates the reads again — k <= 31: the whole input is counted twice, once for the
 *       sizes A's layout depends on, once to write it; k > 31: each pass's columns are staged and concatenated at the end) — bounded by device
 *       memory (16 bytes per instance of the largest pass for k <= 17, 32 for 19 <= k <= 31, 80 / 96 for two- / three-word k-mers, whose
 *       columns are also staged) and by nnz(A) < 2^32 per context (32-bit row / column pointers).  For k > 31 the sort also takes passes, whatever
 *       this option says, when one pass would not fit the device memory free as elba_count_kmers starts (its workspace, 92 / 108 bytes per
 *       instance, and the columns at their largest), or at 2^32 instances; a single 24-bit prefix that holds 2^32 instances or whose pass does
 *       not fit fails with ELBA_ERR_UNSUPPORTED / ELBA_ERR_OUT_OF_MEMORY, naming it.  Tests set a small value to force passes; the result does not
 *       depend on it.  What still holds 32-bit places and refuses more than 2^32 instances with ELBA_ERR_UNSUPPORTED: 19 <= k <= 31 with
 *       UPPER > 255, option "kmer_no_msd", and elba_set_kmer_matrix_device (triples).
 *   "polish_trace_bytes" (>= 0): elba_polish_contigs aligns its voters in batches of consecutive reads whose choices (n * band / 4 bytes per
 *       voter) fit this many bytes; a read that alone exceeds it is a batch of its own.  0, the default: an eighth of the device memory free
 *       as the call starts, at least 64 MiB.  Tests set a small value to force batches; the result does not depend on it.
 *   "measure_prep" (0 | 1): diagnostic — elba_count_kmers runs its emit kernels a second time without what they write for the SpGEMM's sake alone and
 *       brackets both runs with events (elba_get_stat "spgemm_prep_us").
 *   "tune1" .. "tune5", "tune7": A/B switches of the round in progress (what each means is said where the library reads it); never a result-changing switch. */
int  elba_set_option(elba_ctx *ctx, const char *name, int64_t value);
/* Diagnostic counters of the last stage call by name (unknown name: ELBA_ERR_INVALID_ARG); none of them is part of a result.
 *   "overlap_mirror_placed"  mirrored entries of the last elba_create_seed_matrix call that waited in the staging area for the placement pass
 *                            instead of going straight to their row's slab ("mirror slabs")
 *   "overlap_slab_q16"       slab entries reserved per row entry of A in that call, x 65536 (0: the call ran without slabs)
 *   "resident_bytes_A"       device bytes the resident k-mer matrix occupies (CSR, columns, padded column store in use, pointers)
 *   "kmer_path"              how the last elba_count_kmers counted: 0 = sort, 1 = two-level value partition + LDS count tables (k <= 17),
 *                            2 = two-level partition of 16-byte records + LDS sort per bucket (19 <= k <= 31)
 *   "triples_path"           how the last elba_set_kmer_matrix_device built the matrix: 1 = two-level partition by column + the k-mer stage's
 *                            bucket kernels (matrices of some size whose columns all hold entries), 0 = radix sorts of the whole matrix
 *   "padded_columns"         1: the resident matrix has its padded column store (what the fast SpGEMM paths gather from); 0: columns longer than 64
 *                            entries, or the store did not fit a third of the free device memory when the matrix was built
 *                            (elba_release_workspace on other contexts of the device, then build again)
 *   "gather_slots"           columns of the padded column store in use (with inline partners: only the columns some row entry still fetches)
 *   "kmer_passes"            value-range passes the last elba_count_kmers took, either partition path (1: the whole input at once; option "kmer_batch_instances")
 *   "kmer_largest_pass"      instances of its largest value-range pass (a pass holds whole first digits: it may exceed the cap; I when unbatched)
 *   "kmer_peak_bytes"        k > 31 in value-range passes: device bytes the call's passes and column assembly held at their high point, measured
 *                            (hipMemGetInfo); 0 when the call took one pass
 *   "kmer_crowded_buckets"   buckets it gave up to a crowded path (19 <= k <= 31: the pseudo-bucket path; k <= 17: the windowed bucket kernel)
 *   "kmer_crowded_small"     19 <= k <= 31: crowded buckets whose kept entries (0 < Z <= the emit kernels' largest class) would fit an ordinary emit
 *   "kmer_buckets"           buckets of the value partition, summed over the passes (0: the sort) — with kmer_crowded_buckets (summed too), the share
 *                            of buckets that took a crowded path
 *   "overlap_passes"         passes the last elba_create_seed_matrix call took (1: no repeat; also set when the call failed)
 *   "overlap_forwarded"      rows that call forwarded to a larger table tier on its in-call prediction (cold calls without a sample), all passes
 *   "overlap_tier_limit_0" .. "_4"   of the last elba_create_seed_matrix, from its final pass: the claimed table slots at which a row abandons LDS tier t
 *                            (512 << t slots) for the next one — min(3/4 of the slots, slots - lanes of the tier's workgroup) - 1 for the family that ran
 *   "overlap_tier_queued_0" .. "_5"  rows queued on tier t (5: the HBM tables) in that pass: by the classification, forwarded or handed on by the tier below
 *   "overlap_tier_done_0" .. "_5"    rows that completed on tier t (a cold call's sample rows count on tier 3); the sums over t are rows_lds + rows_global
 *   "overlap_sort_rows_bucket", "overlap_sort_rows_huge"
 *                            rows of B whose columns the workgroup bucket sort (1025 .. 4096 entries) and the HBM sort (more) ordered
 *   "overlap_family"         the kernel family of that call: 0 dense path, 1 64-bit accumulators that carry both positions, 2 32-bit accumulators
 *   "overlap_pay16"          1: its 32-bit accumulators carried the partner's position (positions and product sequence numbers fit 16 bits)
 *   "overlap_rec16"          1: staged and mirrored entries were 16-byte records, 0: 32-byte ones
 *   "matrix_col_stride"      of the resident k-mer matrix: entries per column of the padded column store (0: columns are read through their pointers)
 *   "matrix_fbits"           bits of the place-in-column field of a product sequence number
 *   "matrix_pos16"           1: every position is below 65536
 *   "matrix_hints", "matrix_inline", "matrix_suffix"
 *                            1: the row entries carry ownership hints above their position (positions below 2^30) | inline partners | their
 *                            column's length and their place in it (the dense path: some column holds more than 16 entries)
 *   "matrix_csr_words"       1: the rows were built by the sort of one 64-bit word per entry, 0: by the sort of (row, entry) pairs
 *   "spgemm_prep_us"         option "measure_prep": device microseconds the emit kernels of the last elba_count_kmers spent on hint bits, inline partners,
 *                            gather slots and padded columns (the kernels as built minus the same kernels without them; -1: not measured)
 *   "emit_us"                ... and the emit kernels as built
 *   "contig_count", "contig_cycles", "contig_circular", "contig_singletons", "contig_reads", "contig_bases", "contig_branches"
 *                            the last elba_generate_contigs[_ex], under the condition of the contig exports: 0 when the string graph or its
 *                            contigs are not valid ("contig_rank_us": -1)
 *   "graph_segments", "graph_candidates", "graph_links", "graph_closures", "graph_twisted", "graph_unplaced", "graph_clamped", "graph_asymmetric"
 *                            the last elba_export_assembly_links, under the same condition (0 also before the first call on these contigs)
 *   "cc_components", "cc_used_components", "cc_largest_reads", "cc_passes"
 *                            the last elba_graph_components / elba_partition_components: 0 once the graph it labelled is no longer valid
 *   "induce_reads", "induce_pairs", "induce_split_pairs"
 *                            the last elba_induce_part that succeeded (0 before the first)
 *   "text_tile_bytes", "text_scan_span"
 *                            constants of elba_set_reads_text: the bytes of the chunk one workgroup takes per trip of its two passes, and the
 *                            elements one workgroup of its scans covers (longer arrays make the scan recurse) */
int  elba_get_stat(elba_ctx *ctx, const char *name, int64_t *value);

/* Gives the stage calls' scratch memory back to the device (the sort / partition buffers of elba_count_kmers, elba_create_kmer_matrix and
 * elba_set_kmer_matrix_device: ~32 bytes per k-mer instance, 64 GB on BASELINE config 3), keeping the resident matrices, the reads and the
 * buffers of elba_create_seed_matrix.  A caller that builds A once and multiplies many times (or runs a second context beside this one)
 * calls it after elba_create_kmer_matrix; the next stage call allocates again.  The sort keys elba_count_kmers left for
 * elba_create_kmer_matrix go with the scratch: a later elba_create_kmer_matrix rebuilds them from the columns.
 * ELBA_ERR_STATE on a context that counted exchanged records (elba_dist_count_records) or inside a sharded multiplication. */
int  elba_release_workspace(elba_ctx *ctx);

/* ---- distributed building blocks (one context per rank/GPU; the collectives are issued by the host driver) ----------------
 * They replace, for a 1D read-row partition over the GPUs of one node, what the reference does with MPI inside the same four
 * functions: the two k-mer all-to-alls (src/KmerOps.cpp:117-151, :244-274), the k-mer id Exscan (:371-375), and the
 * redistribution of A / AT to their consumers (SpParMat ctor :396-400, Transpose src/main.cpp:272-273).
 * Exchange #1 records: (packed canonical k-mer, global read id << 32 | pos) — W + 1 uint64 words, W = words per k-mer (1 for k <= 31,
 * 2 up to 63, 3 up to 95; NLONGS of include/Kmer.hpp:95-97), most significant word first.
 * Exchange #2 records: two words, (global k-mer id, global read id << 32 | pos), a column's entries contiguous and ordered by (read,pos). */
#define ELBA_MAX_RANKS 64
/* The reference's own k-mer hash and owner on the device: Kmer::GetHash (src/Kmer.cpp:207-213: h1 of murmurhash3_x64_128, seed 313, over
 * the 8 * NLONGS key bytes) and GetKmerOwner (src/KmerOps.cpp:352-359: (size_t)(double(h) * nprocs / double(UINT64_MAX))).  kmers: n
 * packed k-mers of W = NLONGS adjacent words each (first word first); hash / owner: host outputs, either may be NULL. */
int  elba_kmer_hash_owner(elba_ctx *ctx, const uint64_t *kmers, int64_t n, int nprocs, uint64_t *hash, int32_t *owner);

/* Owners by VALUE RANGE.  The value space of the packed canonical k-mers is cut into ELBA_OWNER_BINS equal bins (leading 12 bits of the
 * first word); elba_dist_value_histogram counts this rank's instances per bin; the driver all-reduces the histograms, picks boundaries
 * that balance the instances and announces them with elba_dist_set_owner_ranges: rank r owns the bins [upper_bins[r-1], upper_bins[r]),
 * upper_bins[nranks-1] == ELBA_OWNER_BINS.  (The reference hashes, GetKmerOwner src/KmerOps.cpp:352-359; with ranges the owners'
 * reliable k-mers are disjoint ascending runs, so the global k-mer id — rank of the value — is the owner's local index plus the
 * exclusive scan of the owners' counts, the reference's MPI_Exscan of src/KmerOps.cpp:371-375: elba_dist_set_kmer_id_base.) */
#define ELBA_OWNER_BINS 4096
int  elba_dist_value_histogram(elba_ctx *ctx, uint64_t *hist, int64_t nbins);
int  elba_dist_set_owner_ranges(elba_ctx *ctx, int nranks, const uint32_t *upper_bins);
/* after elba_dist_count_records: global id of this owner's i-th reliable k-mer = base + i; nall = reliable k-mers of all owners */
int  elba_dist_set_kmer_id_base(elba_ctx *ctx, int64_t base, int64_t nall);
/* instances of this rank's reads per owner rank */
int  elba_dist_count_owners(elba_ctx *ctx, int nranks, uint64_t *counts);
/* write this rank's records into d_send (device, 8 (W + 1) bytes per record) grouped by owner; offsets[r] = first record index of owner r */
int  elba_dist_fill_send(elba_ctx *ctx, int nranks, void *d_send, const uint64_t *offsets);
/* Exchange #1 with 8-byte records (one-word k-mers, k <= 31; round 5).  The reference ships (k-mer, read, pos) per instance
 * (src/KmerOps.cpp:105-151: a k-mer of NBYTES + the 8-byte seed, batched); here an instance travels as
 * (value - first value of the owner's range) << index_bits | instance index in the SENDER's reads — the source rank is the segment of the
 * receive buffer a record arrives in — where value_bits + index_bits <= 64 (k = 17 at two or more ranks of BASELINE config 3; never k = 31).
 * elba_dist_packed_format: read_bounds[nranks + 1] = first global read of every rank, all_lens = the lengths of ALL reads (one all-gather of
 * 4 bytes per read); decides the format — the same on every rank — and stores every rank's instance offsets on the device; *fits = 0: keep
 * elba_dist_fill_send's 16-byte records.  Call after elba_dist_set_owner_ranges.  elba_dist_fill_send_packed: as elba_dist_fill_send, 8 bytes
 * per record.  elba_dist_unpack_records: the owner side — recv_counts[p] packed records of rank p, segment after segment in d_packed, become
 * 16-byte records (k-mer, global read << 32 | pos) in d_records, what elba_dist_count_records takes; `rank` = this owner. */
int  elba_dist_packed_format(elba_ctx *ctx, int nranks, const int64_t *read_bounds, const uint32_t *all_lens, int *fits, int *value_bits, int *index_bits);
int  elba_dist_fill_send_packed(elba_ctx *ctx, int nranks, void *d_send, const uint64_t *offsets);
int  elba_dist_unpack_records(elba_ctx *ctx, int nranks, int rank, const void *d_packed, const uint64_t *recv_counts, void *d_records);
/* owner side: exact count + [lower, upper] filter of the received records; builds the owner's columns (device; records are
 * borrowed until elba_dist_set_global_kmers returns) */
int  elba_dist_count_records(elba_ctx *ctx, const void *d_records, int64_t nrecords, elba_kmer_stats *stats);
/* device pointer to this owner's reliable k-mers, ascending (input of the all-gather); one-word k-mers only */
int  elba_dist_get_reliable_kmers(elba_ctx *ctx, const void **d_kmers, int64_t *n);
/* copy them into a caller-owned device buffer of at least W * capacity words, the W words of a k-mer adjacent (e.g. a torch tensor that
 * takes part in the all-gather); capacity counts k-mers */
int  elba_dist_copy_reliable_kmers(elba_ctx *ctx, void *d_dst, int64_t capacity);
/* alternative to elba_dist_set_kmer_id_base for owners that are not value ranges: all owners' reliable k-mers concatenated (any order;
 * nall k-mers of W adjacent words): global k-mer id = rank of the packed value */
int  elba_dist_set_global_kmers(elba_ctx *ctx, const void *d_all_kmers, int64_t nall);
/* column panels: read_bounds[r] = first global read id of rank r (read_bounds[nranks] = total reads).  counts[r] = records this
 * owner sends to rank r: every column, whole, for every rank that owns at least one of its reads */
int  elba_dist_panel_counts(elba_ctx *ctx, int nranks, const uint64_t *read_bounds, uint64_t *counts);
int  elba_dist_panel_fill(elba_ctx *ctx, int nranks, const uint64_t *read_bounds, void *d_send, const uint64_t *offsets);
/* Row-block batching: the same with one ROW BLOCK per rank, [win_lo[r], win_hi[r]) inside rank r's rows — a column goes to rank r only
 * if it has a read in that block.  A rank whose whole panel would not fit (dense columns: nearly every column reaches every rank, cf.
 * the reference's batched exchange, include/KmerOps.hpp:33-56) walks its rows block by block: panel_*_win -> all-to-all ->
 * elba_dist_set_panel(block) -> elba_create_seed_matrix -> rows of the block -> next block.  The owner's columns stay resident. */
int  elba_dist_panel_counts_win(elba_ctx *ctx, int nranks, const uint64_t *read_bounds, const uint64_t *win_lo, const uint64_t *win_hi, uint64_t *counts);
int  elba_dist_panel_fill_win(elba_ctx *ctx, int nranks, const uint64_t *read_bounds, const uint64_t *win_lo, const uint64_t *win_hi, void *d_send, const uint64_t *offsets);
/* create_seed_matrix on a row shard WITH mirror exchange.  elba_create_seed_matrix on a shard accumulates every pair that has a row
 * outside the shard on both ranks concerned (no communication, about twice the accumulator work and table sizes of a one-GPU run).  The
 * three calls below accumulate each pair {i, j} on ONE rank — the rank of the smaller row when i + j is even, of the larger when odd —
 * and hand the mirrored entry to the other: begin (classify + numeric; send_counts[r] = 32-byte records for rank r), fill (writes them
 * grouped by rank at offsets[r]), the driver's all-to-all, end (merges what arrived, row pointers, per-row column sort: this rank's rows of
 * B are then complete, exactly as after elba_create_seed_matrix).  read_bounds as in elba_dist_panel_counts.  The only exchange inside
 * the reference's create_seed_matrix this corresponds to are the SUMMA stages of Mult_AnXBn_DoubleBuff (src/SharedSeeds.cpp:7). */
int  elba_seed_matrix_begin(elba_ctx *ctx, int nranks, const uint64_t *read_bounds, uint64_t *send_counts);
int  elba_seed_matrix_fill(elba_ctx *ctx, void *d_send, const uint64_t *offsets);
int  elba_seed_matrix_end(elba_ctx *ctx, const void *d_recv, int64_t nrecords, elba_overlap_stats *stats);
/* The same step with ONE host synchronisation — nothing about the exchange has to be known on the host:
 *   elba_set_stream         the library launches on the caller's HIP stream from now on (the stream its collectives are ordered against)
 *   elba_seed_matrix_send   queues classify + numeric + the grouping of the cross-rank mirror images into d_send = nranks slots of slot_records
 *                           32-byte records: record 0 of slot r is a header written on the device (count, "repeat" flag, slot size needed), the
 *                           images for rank r follow.  Does not wait.
 *   (the driver's all-to-all with EQUAL splits: slot r of d_send -> slot <this rank> of rank r's d_recv)
 *   elba_seed_matrix_recv   queues the merge of d_recv's slots (d_recv is scratch: tickets are written into it), row pointers, column sort;
 *                           synchronises once.  ELBA_OK: this rank's rows of B are complete.  ELBA_ERR_RETRY: this rank's staging area or some
 *                           rank's slot was too small — the flag travels in every header, so every rank gets this answer in the same step —
 *                           capacities have grown: repeat send / all-to-all / recv with *slot_records_needed (the same value on every rank).
 *                           With ELBA_OK *slot_records_needed is the slot size this step would have got by with (+ 1/8; <= slot_records, again
 *                           the same on every rank): a caller whose first guess was generous uses it for its next step — whole slots travel. */
int  elba_set_stream(elba_ctx *ctx, void *hip_stream);
int  elba_seed_matrix_send(elba_ctx *ctx, int nranks, const uint64_t *read_bounds, void *d_send, int64_t slot_records);
int  elba_seed_matrix_recv(elba_ctx *ctx, void *d_recv, int64_t slot_records, elba_overlap_stats *stats, int64_t *slot_records_needed);
/* receiver side: the panel of every column touching rows [row_lo,row_hi) -> columns (renumbered by rank among the columns present) + CSR; elba_create_seed_matrix
 * then computes exactly those rows of B (global column ids); elba_export_csr(row_lo,row_hi) / elba_export_dcsc read them */
int  elba_dist_set_panel(elba_ctx *ctx, const void *d_records, int64_t nrecords, int64_t nreads_total, int64_t nkmers_total,
                         int64_t row_lo, int64_t row_hi, elba_matrix_stats *stats);

#ifdef __cplusplus
}
#endif
#endif /* ELBA_AMD_H_ */
