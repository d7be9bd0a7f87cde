// Internal declarations shared by the HIP translation units of libelba_amd.so.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <new>
#include <string>
#include <vector>
#include "../../include/elba_amd.h"
#include "state.hpp"
#include "msd_plan.hpp"

namespace elba {

struct Error {
    int code;
    std::string msg;
};

#define ELBA_HIP(expr)                                                                                   \
    do {                                                                                                 \
        hipError_t e__ = (expr);                                                                         \
        if (e__ != hipSuccess) {                                                                         \
            throw ::elba::Error{e__ == hipErrorOutOfMemory ? ELBA_ERR_OUT_OF_MEMORY : ELBA_ERR_HIP,      \
                                std::string(#expr) + ": " + hipGetErrorString(e__) + " (" + __FILE__ +  \
                                    ":" + std::to_string(__LINE__) + ")"};                               \
        }                                                                                                \
    } while (0)

#define ELBA_REQUIRE(cond, code, text)                       \
    do {                                                     \
        if (!(cond)) throw ::elba::Error{(code), (text)};    \
    } while (0)

// Work that must run once per DEVICE and process (hipFuncSetAttribute applies to the current device: a host process that drives two GPUs, or
// ranks that run as threads, must each set it on their own device) — serialised, so that threads never race on the flags.
struct DeviceOnce {
    std::mutex m;
    bool done[64] = {};
    template <class F> void run(int dev, F &&f)
    {
        std::lock_guard<std::mutex> g(m);
        if (dev >= 0 && dev < 64 && done[dev]) return;
        f();
        if (dev >= 0 && dev < 64) done[dev] = true;
    }
};

// Growable device buffer (never shrinks; capacity is reused across calls so the steady state allocates nothing).
struct DevBuf {
    void *p = nullptr;
    size_t cap = 0;
    ~DevBuf() { release(); }
    DevBuf() = default;
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    void release()
    {
        if (p) (void)hipFree(p);
        p = nullptr;
        cap = 0;
    }
    void reserve(size_t bytes)
    {
        if (bytes <= cap) return;
        release();
        size_t want = bytes + (bytes >> 3) + 256;   // slack so that small growth does not reallocate
        hipError_t e = hipMalloc(&p, want);
        if (e != hipSuccess) { want = bytes; e = hipMalloc(&p, want); }
        if (e != hipSuccess) { p = nullptr; throw Error{ELBA_ERR_OUT_OF_MEMORY, "hipMalloc of " + std::to_string(bytes) + " bytes failed"}; }
        cap = want;
    }
    void reserve_exact(size_t bytes)      // (no slack: buffers that are filled once, at a size known in advance)
    {
        if (bytes <= cap) return;
        release();
        const hipError_t e = hipMalloc(&p, bytes);
        if (e != hipSuccess) { p = nullptr; throw Error{ELBA_ERR_OUT_OF_MEMORY, "hipMalloc of " + std::to_string(bytes) + " bytes failed"}; }
        cap = bytes;
    }
    template <class T> T *as() const { return reinterpret_cast<T *>(p); }
    void swap(DevBuf &o) { void *tp = p; p = o.p; o.p = tp; size_t tc = cap; cap = o.cap; o.cap = tc; }
};

struct EventTimer {
    hipEvent_t a = nullptr, b = nullptr;
    void init() { if (!a) { ELBA_HIP(hipEventCreate(&a)); ELBA_HIP(hipEventCreate(&b)); } }
    void start(hipStream_t s) { init(); ELBA_HIP(hipEventRecord(a, s)); }
    void stop(hipStream_t s) { ELBA_HIP(hipEventRecord(b, s)); }
    float ms() { float t = 0; ELBA_HIP(hipEventSynchronize(b)); ELBA_HIP(hipEventElapsedTime(&t, a, b)); return t; }
    ~EventTimer() { if (a) (void)hipEventDestroy(a); if (b) (void)hipEventDestroy(b); }
};

// Phase marks of one call on one stream: N events, one record per phase boundary (every record costs stream time — the overlap
// SpGEMM's whole call is a few hundred microseconds, so boundaries are shared instead of bracketing every phase with its own pair)
template <int N>
struct PhaseMarks {
    hipEvent_t e[N] = {};
    void mark(int k, hipStream_t s) { if (!e[k]) ELBA_HIP(hipEventCreate(&e[k])); ELBA_HIP(hipEventRecord(e[k], s)); }
    float ms(int from, int to) { float t = 0; ELBA_HIP(hipEventSynchronize(e[to])); ELBA_HIP(hipEventElapsedTime(&t, e[from], e[to])); return t; }
    ~PhaseMarks() { for (int k = 0; k < N; ++k) if (e[k]) (void)hipEventDestroy(e[k]); }
};

// ---- primitives (prims.hip) -------------------------------------------------------------------------------------
// Exclusive prefix sums; in and out may alias.  tmp is grown as needed.
void exclusive_scan_u32(hipStream_t s, const uint32_t *in, uint32_t *out, int64_t n, DevBuf &tmp);
void exclusive_scan_u32_to_i64(hipStream_t s, const uint32_t *in, int64_t *out, int64_t n, DevBuf &tmp);
// Stable LSD radix sort of (key u64, value u64) pairs on key bits [bit_lo, bit_hi).  Ping-pongs between the two
// buffer pairs; returns 0 if the result is in (k0,v0), 1 if in (k1,v1).
// hint bits (see Ctx::csr_hints) of the entry of read i in a column of L <= 64 entries (read << 32 | pos)
__device__ __forceinline__ uint32_t column_hint(const uint64_t *col, uint32_t L, uint32_t i, uint32_t win_lo, uint32_t win_hi)
{
    bool own_g = false, own_w = false;
    uint32_t mult = 0;
    for (uint32_t t = 0; t < L; ++t) {
        const uint32_t j = (uint32_t)(col[t] >> 32);
        if (j == i) { ++mult; continue; }
        const bool par = ((i ^ j) & 1u) ? j < i : j > i;
        own_g |= par; own_w |= par || j < win_lo || j >= win_hi;
    }
    if (mult >= 2) return 0u;
    return (own_g ? 0u : 1u) | (own_w ? 0u : 2u);
}
// (HINT_MAX_COL — longer columns are not examined —: msd_plan.hpp, whose rank decision reads it)

int radix_sort_pairs(hipStream_t s, uint64_t *k0, uint64_t *v0, uint64_t *k1, uint64_t *v1, int64_t n, int bit_lo, int bit_hi, DevBuf &tmp);
// The same for bare 64-bit words (whatever rides in the bits outside [bit_lo, bit_hi) moves with them): returns 0 if the result is in k0, 1 if in k1.
int radix_sort_keys(hipStream_t s, uint64_t *k0, uint64_t *k1, int64_t n, int bit_lo, int bit_hi, DevBuf &tmp, bool first_hist_done = false);
int radix_sort_where(int64_t n, int bit_lo, int bit_hi);
// The CSR build's sort of one-word keys (read << rs | id << (pb + 2) | hint << pb | pos, or an inline partner: bit 63, matrix.hip) on the read bits
// [rs, rs + mb), with the LAST pass writing the rows of A themselves: csr[z] = the unpacked entry (k_unpack_csr_words' format) and rowptr[0 .. M]
// (the first entry of every read, empty rows included) — no pass over the sorted keys behind the sort.  The keys in k0 are consumed.
struct CsrFin { int idbits, pb, rs, mb, pbi; uint64_t *csr; uint32_t *rowptr; int64_t M; };
void radix_sort_keys_to_csr(hipStream_t s, uint64_t *k0, uint64_t *k1, int64_t n, const CsrFin &f, DevBuf &tmp);
int radix_sort_pairs_k32(hipStream_t s, uint32_t *k0, uint64_t *v0, uint32_t *k1, uint64_t *v1, int64_t n, int bit_lo, int bit_hi, DevBuf &tmp);
void group_offsets_k32(hipStream_t s, const uint32_t *sorted_keys, int64_t n, uint32_t *ptr, int64_t nkeys);
void radix_column_scan(hipStream_t s, uint32_t *rows, int64_t nrows, uint32_t nbins, DevBuf &tmp);      // (prims.hip)
uint32_t *radix_first_histogram(int64_t n, int bit_lo, int bit_hi, DevBuf &tmp, int *shift, int *bits, int *tile);      // (prims.hip)
void fill_u32(hipStream_t s, uint32_t *p, uint32_t v, int64_t n);
void fill_u64(hipStream_t s, uint64_t *p, uint64_t v, int64_t n);
// ptr[k] = first index z with keys[z] >= k, for k in [0, nkeys]; keys ascending (sorted group ids -> CSR/CSC pointers)
void group_offsets_u32(hipStream_t s, const uint64_t *sorted_keys, int key_shift, int64_t n, uint32_t *ptr, int64_t nkeys);
uint64_t reduce_max_u64(hipStream_t s, const uint64_t *p, int64_t n, DevBuf &tmp);   // synchronises
int64_t scan_block_span();      // elements one workgroup of the scans covers: beyond it they recurse (elba_get_stat "text_scan_span")

// ---- tuning and A/B switches (elba_set_option) --------------------------------------------------------------------------
// Every default is the production path and none of them changes a result: the alternatives are kept for measurements and for the parity
// tests that walk them.  They used to be environment variables read inside the stages; a library does not read its caller's environment.
struct Options {
    bool no_symmetry = false;   // SpGEMM: accumulate both triangles instead of one + mirror
    bool no_ell = false;        // plain CSC columns instead of the padded column store
    bool no_pay = false;        // 32-bit accumulators + seed look-ups instead of the position-carrying 64-bit ones
    bool mir32 = false;         // 32-byte staging / mirror records instead of 16-byte words
    bool no_hints = false;      // no ownership bits in the rows of A
    bool no_sample = false;     // a cold call does not compute a sample of rows first
    bool no_ell_compact = false;// k-mer stage: the padded column store holds every column, row entries name k-mer ids (no gather slots)
    bool no_slab = false;       // SpGEMM: mirrored entries wait in the staging area for k_mirror instead of going straight to their row's slab (spgemm.hip: "mirror slabs")
    bool csr_pairs_late = false; // dense matrices from the two-level partition: the CSR build's sort pairs written by the CSR build, not by the bucket kernels (A/B)
    bool msd_rank = false;      // k-mer stage: column ranks whatever UPPER is (tests)
    bool msd_no_rank = false;   // k-mer stage: entries without their column's rank — the emit kernels sort by ranges of the 16 value bits (A/B; what runs when the payload leaves no room)
    int ell_slot_cap = 0;       // test hook: the padded column store pretends to hold this many gather slots only (0: its real size)
    int slab_pct = 175;         // SpGEMM: a row's slab holds this many percent of the mirrored entries the measured ratio predicts for it (+ SLAB_PAD)
    int slab_q16 = 0;           // test hook: slab entries per row entry of A in 1/65536 units, instead of the measured ratio (small matrices take no sample)
    bool panel_inline = false;  // inline partners in the rows of a windowed matrix too (a shard's panel): such a matrix is multiplied with the mirror exchange only
    bool no_inline = false;     // no inline partners in the rows of A (the owner's entry of a two-read column carries the other read: no column fetch)
    bool no_suffix = false;     // dense matrices stay on the general kernel
    bool ov_generic = false;    // SpGEMM: reads-built matrices take the general numeric kernel, not its reads-path instantiation (A/B; option "ov_generic" = 1)
    bool ov_spec_rt_geom = false;      // SpGEMM: the reads path keeps its run-time geometry, not the compiled-geometry instantiation (A/B; option "ov_generic" = 2)
    bool no_row_order = false;  // dense matrices: partners are named by their row, not by a label that brings reads of one locus together
    bool kmer_pairs = false;    // (value, payload) pairs through the k-mer sort instead of one packed word
    bool kmer_unfused = false;  // per-head column emission (k_runs<true> + k_instance_entries) instead of k_runs_emit
    bool kmer_msd = false;      // force the two-level partition path on inputs below its size threshold (tests)
    bool kmer_no_msd = false;   // k <= 17: keep the LSD sort of the whole value instead of the two-level partition + LDS count (kmer_msd.hip)
    bool csr_pairs = false;     // (read, entry) pairs through the CSR sort instead of one word
    bool emit_plain = false;    // k-mer emit without the fused first histogram
    bool trace = false;         // progress lines on stderr
    bool measure_prep = false;  // diagnostic (bench.py, "spgemm_prep"): elba_count_kmers runs its emit kernels a second time WITHOUT what they write for the SpGEMM's sake alone (hint bits,
                                // inline partners, gather slots + padded columns), both runs bracketed by events: elba_get_stat("spgemm_prep_us") = the difference (kmer_msd.hip)
    int64_t tune[8] = {0, 0, 0, 0, 0, 0, 0, 0};      // A/B switches ("tune1" .. "tune5", "tune7"; entries 0 and 6 are retired and stay zero): what each means is said where it is read
    int msd_wide_bits = 0;      // tests: value bits the partition of the 19 <= k <= 31 path takes (0: chosen from the number of instances; batched: each pass's, at least 11 + its first level's extra bits)
    int64_t kmer_batch_instances = 0;      // k-mer stage (reads, k >= 9): more instances than this are counted in passes over value ranges (0: 0xE0000000 — what a 32-bit place holds; k > 31: also no more than the device memory holds); tests force passes on small sets
    int msd_small_cap = 0;      // tests: buckets with more entries than this go to the crowded-bucket kernel (0 = its real capacity)
    int kmer_drop = 0;          // test hook: force that many dropped index bits on a small input (1..3)
    int dense_up = 1;           // SpGEMM, dense path: the tier its rows start on at least (1: eight wavefronts share a 1024-slot table — 32 per CU as with four on 512 slots, half the load)
    int dense_wgs = 8;          // SpGEMM, dense path: workgroups of the 512-slot tier per CU
    int dk = -1;                // SpGEMM: gather trips per iteration of the padded-column loop: 0 = one, 1 = two, 2 = four, 4 = eight; -1 = chosen per matrix (spgemm.hip)
    int64_t aln_tiers = 0;      // x-drop register tiers as decimal digits (1248 = all), 0 = default
    int aln_wide_hint = 6, aln_long_hint = 6000;
    int64_t polish_trace_bytes = 0;      // elba_polish_contigs: the choices of one batch of voters take at most this many bytes (0: an eighth of the free device memory, at least 64 MiB); tests force batches on small sets
};

// ---- context ----------------------------------------------------------------------------------------------------
// the rows [lo, hi) of B a context computes (Ctx::window)
struct RowWindow { int64_t lo, hi; int64_t rows() const { return hi - lo; } };

// an entry of the symmetrised R that tr.hip builds and leaves in Ctx::tr_sym (CSR over the reads, Ctx::tr_ptr; columns ascending within a row):
// meta = direction | directionT << 3 | below-diagonal << 6.  stars.hip looks columns up in it
struct alignas(16) SymEntry { uint32_t col; int32_t suffix, suffixT; uint32_t meta; };
static_assert(sizeof(SymEntry) == 16, "tr.hip and stars.hip read 16-byte entries");

// The buffer set of the pileup's keys-to-segments sequence (pileup.hip: depth_segments), owned by each stage that runs it (Ctx::pu, and Ctx::pl
// so that place.hip runs the same launches on buffers of its own).  seg_off / seg_start / seg_depth are what the sequence leaves, the rest is scratch
struct DepthBufs {
    DevBuf k0, k1, eptr, head, hidx, delta, dsum, gstart, tok, tpos, seg_off, seg_start, seg_depth;
    void reserve(int64_t max_keys, int64_t G);      // for at most max_keys endpoints of G groups (pileup.hip)
    void release_scratch() { for (DevBuf *b : {&k0, &k1, &eptr, &head, &hidx, &delta, &dsum, &gstart, &tok, &tpos}) b->release(); }
    void release() { release_scratch(); seg_off.release(); seg_start.release(); seg_depth.release(); }
};

struct Ctx {
    elba_cfg cfg{};
    Options opt;
    int device = 0;
    hipStream_t stream = nullptr;
    std::string last_error;
    int num_cus = 256;
    Validity v;                            // which of the products below are valid: state.hpp decides, the stages name their event

    // reads (DnaBuffer layout)
    int64_t nreads = 0, first_global_id = 0, packed_bytes = 0;
    const uint8_t *d_packed = nullptr;     // either owned (own_*) or borrowed from the caller
    const uint64_t *d_byte_off = nullptr;
    const uint32_t *d_len = nullptr;
    DevBuf own_packed, own_byte_off, own_len;
    uint32_t max_read_len = 0;             // longest read (set by stage_count_kmers)
    std::vector<uint32_t> h_len;           // host copy of lengths (instance offsets are a host-side prefix sum)
    std::vector<uint64_t> h_byte_off;
    // the index of reads that came in as text (text_index.hip): .fai records and name extents, device and host copy.  It belongs to the read
    // set like its lengths: tx_index is true only while the reads of that elba_set_reads_text call are the context's (reads_replaced)
    bool tx_index = false;
    DevBuf tx_recs, tx_name_pos, tx_name_len;      // elba_fasta_record_t[nreads], u64[nreads], u32[nreads]
    std::vector<elba_fasta_record_t> tx_h_recs; std::vector<uint64_t> tx_h_name_pos; std::vector<uint32_t> tx_h_name_len;

    // k-mer stage results (device)
    int triples_path = 0; // diagnostic: how the last elba_set_kmer_matrix_device built the matrix — 0 radix sorts of the whole matrix (matrix.hip), 1 the k-mer stage's bucket kernels (kmer_msd.hip)
    int kmer_passes = 1;  // diagnostic: value-range passes of the last elba_count_kmers (kmer_msd.hip)
    int64_t kmer_crowded = 0, kmer_crowded_small = 0, kmer_largest_pass = 0;      // diagnostic: the last elba_count_kmers' crowded buckets, wide ones of them with a folded entry count in (0, small_cap], instances of its largest pass (kmer_msd.hip)
    int64_t kmer_peak_bytes = 0;   // diagnostic: device bytes the last elba_count_kmers held at its high point, measured (value-range passes of k > 31; 0 otherwise)
    int64_t kmer_buckets = 0;      // diagnostic: buckets of the last elba_count_kmers' value partition, summed over its passes (kmer_msd.hip; 0: the sort)
    int kmer_path = 0;    // diagnostic: how the last elba_count_kmers counted — 0 the sort of kmer.hip, 1 two-level partition + LDS count tables (k <= 17), 2 the same on 16-byte records + LDS sort (19 <= k <= 31)
    int64_t I = 0, ndistinct = 0;
    DevBuf inst_off;      // u64[M+1] instance offset of each read
    DevBuf rel_kmers;     // u64[N] reliable k-mers ascending (right-aligned value order == packed order)
    DevBuf rel_kmers_lo;  // u64[N] their second word when k > 32
    DevBuf rel_kmers_lo2; // u64[N] their third word when k > 64
    DevBuf rel_counts;    // u32[N]
    DevBuf csr_words;     // u64[Z] the CSR build's sort key of every entry of a_csc — read << pre.rs | k-mer id << (pre.pb + 2) | hint << pre.pb | pos, or an inline partner (csr_plan.hpp) — when pre.words
    CsrHandoff pre;       // what the k-mer stage (k_runs_emit's caller in kmer.hip, the bucket kernels of kmer_msd.hip — for reads and for device triples) leaves for the CSR build of
                          // the same matrix: assigned whole by the producer, reset where elba_count_kmers starts, consume()d by the build that used it and by elba_release_workspace
    // The format of the resident A — csr_hints, csr_inline, csr_inline_window, csr_one_word, csr_suffix, pos16, j_shift, have_row_order below — is decided by
    // plan_csr_build (csr_plan.hpp) and assigned in ONE place, when the build has run (matrix.hip: CsrBuild::publish_format).
    // Ownership hints of the SpGEMM, two bits in every a_csr entry (kid << 32 | hint << 30 | pos; positions below 2^30): bit 30 = under the
    // parity rule of owns_pair (spgemm_direct.hpp) this row accumulates NO pair of the entry's column and appears in it once — the column
    // need not be fetched at all, the entry only counts one diagonal product; bit 31 = the same with every partner outside the row window
    // counted as owned (calls without the mirror exchange between ranks).  They are a property of A, written when A is built (k_runs_emit /
    // k_csc_to_csr_words: every entry sees its whole column there anyway).  csr_hints false: both bits are zero / positions use all 32 bits.
    bool csr_hints = false, ov_hints_used = false, ov_rec16 = false;
    // Inline partners (whole-matrix windows, positions below 2^16, read ids and positions narrow enough for one sort word): four in five columns of
    // 15 %-error reads hold TWO reads, and under the parity rule exactly one of the two rows accumulates the pair (of longer columns: an entry whose
    // row accumulates exactly ONE pair of the column).  That row's entry then carries the pair itself — a_csr entry = 1 << 63 | (partner >> 1) << 32 | posQ | posT << 16, the partner's low bit follows from the rule — and the SpGEMM
    // fetches no column for it (58 % of its gathers on BASELINE config 3).  Such an entry has no k-mer id: exports rebuild CSR from the columns.
    bool csr_inline = false;
    bool csr_inline_window = false;      // ... written for a matrix with a row window (option "panel_inline"): valid under the parity rule over all rows only, i.e. for calls with the mirror exchange
    bool csr_one_word = false;  // diagnostic (elba_get_stat "matrix_csr_words"): the one-word CSR sort built the rows of the resident A, not the key/value pair sort
    bool csr_suffix = false;  // dense matrices: a_csr entries are kid << 32 | column length << 23 | own place in the column << 16 | pos, pairs owned by the smaller row (matrix.hip)
    DevBuf ov_sample;         // u32[256]: the rows a cold SpGEMM call computes first (spgemm.hip)
    int64_t A_products = 0;   // sum over the window's row entries of their column's length (what the SpGEMM reports as `products`)
    DevBuf prod_ctr;
    DevBuf kid_of_entry;  // u64[Z] k-mer id of every entry of a_csc (written with the columns; what the CSR build sorts by read)
    elba_kmer_stats kstats{};

    // A (device)
    bool A_has_kmers = false;
    int64_t M = 0, N = 0, Z = 0, max_row_nnz = 0, max_col_nnz = 0;
    DevBuf a_rowptr, a_csr, a_colptr, a_csc;   // u32[M+1], u64[Z], u32[N+1], u64[Z]
    DevBuf a_ell;                              // u64[N * s_stride]: the columns padded to a common stride (entries, then all ones) — the column store the
                                               // SpGEMM gathers from when no column is longer than 64 entries: column kid starts at kid * s_stride, no pointer
    bool use_ell = false;
    // gather slots (kmer_msd.hip, BucketOut): with inline partners the padded store holds only the columns some row entry still fetches; such an entry
    // names its column's slot in the id field of its a_csr word (the others keep the k-mer id), ell_slot_kid[slot] = k-mer id.  Not compact: slot == k-mer id.
    bool ell_compact = false;
    int64_t ell_nslots = 0, ell_cap_cols = 0;  // slots in use (compact: an upper bound, chunks are drawn whole) / columns the store was sized for
    DevBuf ell_slot_kid;                       // u32[ell_nslots]
    DevBuf a_ellj;                             // u32[N << j_shift]: the partner reads of every column, right-aligned in an aligned block of 32 or 64 slots (dense matrices, Ctx::csr_suffix)
    DevBuf row_order, row_label, row_keys; bool have_row_order = false;      // u32[M] each, dense matrices: the rows sorted by their smallest k-mer id (label -> row) and its inverse (row -> label); a_ellj then names partners by label
    uint32_t j_shift = 5;
    DevBuf col_w0;                             // u8[N]: rotation of every padded column of a dense matrix with a row window (matrix.hip: k_fill_ell)
    uint32_t s_stride = 4, lpc_log2 = 1;       // padded column stride in entries (4, or a multiple of 8: a whole number of 64-byte lines); lanes of the SpGEMM per row entry 2^lpc_log2 >= s_stride / 2
    bool cold_calls = false;                   // every elba_create_seed_matrix call forgets what earlier calls learned (prior, tier usage): elba_set_option
    bool pos16 = false;                        // every position among the entries is < 65536 (mirrored entries of B travel as 16-byte records then)
    uint32_t fbits = 1;                        // bits of the column-position field of a product sequence number
    int64_t row_lo = 0, row_hi = -1;           // rows of B computed by this context (-1: all)
    RowWindow window() const { return {row_lo, row_hi < 0 ? M : row_hi}; }      // ... resolved
    // rows of an A built from reads are local read indices; exported triples carry global ids (src/KmerOps.cpp:215-219)
    int64_t first_global_id_rows() const { return A_has_kmers ? first_global_id : 0; }

    // distributed owner state (kmer.hip, second half)
    const uint64_t *d_records = nullptr; int64_t nrecords = 0;
    bool dist_owner = false;
    DevBuf dist_gid;          // u32[N_local] global k-mer id of each local column
    int64_t dist_nall = -1;
    DevBuf dist_all_off; std::vector<int64_t> dist_bounds; int dist_pack_vb = 0, dist_pack_ib = 0;      // exchange #1 with 8-byte records (kmer.hip, stage_dist_packed_format): every rank's instance offsets (rank r's at bounds[r] + r), the read bounds, the format
    std::vector<uint32_t> owner_upper;   // value-range owners: rank r owns the value bins [owner_upper[r-1], owner_upper[r]) (kmer.hip)
    int64_t N_global = -1;    // a panel context: k-mers of the whole run (its own columns are renumbered locally)
    DevBuf own_colptr, own_csc;   // the columns this rank OWNS (u32[own_N + 1], u64[own_Z]): kept apart from the context's A, which the panels overwrite —
    int64_t own_N = 0, own_Z = 0; // a rank serves one panel per row block of every rank (elba_dist_panel_*_win)

    // B (device)
    int64_t Y = 0;
    DevBuf b_rowptr, b_col, b_val;             // i64[M+1], u32[Y], elba_seed_t[Y]
    elba_overlap_stats ostats{};

    // alignments (align.hip)
    int64_t naln = 0;
    DevBuf aln_tasks, aln_ext, aln_cnt, aln_ptr, aln_ctr, aln_ofl, aln_scratch, aln_rows, aln_cols, aln_out;
    elba_align_stats astats{};
    DevBuf aln_all_packed, aln_all_off, aln_all_len;     // every read of the run, replicated for a row shard's alignments (elba_dist_set_all_reads)
    int64_t aln_all_n = -1; uint32_t aln_all_maxlen = 0;

    // string graph (tr.hip)
    int64_t tr_in_M = 0, tr_in_n = 0;
    DevBuf tr_in_rows, tr_in_cols, tr_in_vals;
    bool tr_outside = false;               // outside counts are attached to the loaded edge list (elba_set_outside_counts): tr_oa / tr_op, u32[tr_in_M] each
    DevBuf tr_oa, tr_op;
    int64_t tr_M = 0, tr_nnz = 0, tr_id_base = 0;
    DevBuf tr_deg, tr_pas, tr_flags, tr_k0, tr_v0, tr_k1, tr_v1, tr_ptr, tr_sym, tr_src, tr_mark, tr_ctr, tr_sel, tr_out_rows, tr_out_cols, tr_out_vals;
    int64_t tr_sym_M = 0, tr_sym_n = 0;     // what tr_ptr / tr_sym describe since the last reduction that succeeded: reads, symmetrised entries (0: tr_ptr was not written)
    elba_string_stats sstats{};

    // contigs (contig.hip): results (cid, eread, epre, estr, eboff, soff, coff, seq, kind) survive elba_release_workspace, the rest is scratch.
    // serial counts the contig calls: the later stages note in their for_cg which one their counts belong to
    struct ContigStage {
        int64_t n = 0, E = 0, bases = 0, circular = 0, singletons = 0;
        DevBuf ptr, slot, kdeg, far[2], rank[2], mn[2], term, vinfo, flag, cidx, nel, eoff, ctr;
        DevBuf cid, eread, epre, estr, eboff, soff, coff, seq, kind;
        DevBuf cfar[2], crank[2];          // scratch of the second ranking pass (ELBA_CONTIG_CIRCULAR)
        EventTimer t_total, t_rank;
        elba_contig_stats stats{};
        uint64_t serial = 0;
        void release_scratch()
        {
            for (DevBuf *b : {&ptr, &slot, &kdeg, &term, &vinfo, &ctr, &flag, &cidx, &nel, &eoff}) b->release();
            for (int b = 0; b < 2; ++b) { far[b].release(); rank[b].release(); mn[b].release(); cfar[b].release(); crank[b].release(); }
        }
    } cg;

    // assembly links (graph_links.hip): all scratch — the column pointers of S, first / last / strand bits per read, link counts per read and
    // their scan, the counters (per workgroup and summed), the records before they are copied out.  for_cg: the contig call (cg.serial) the counts in stats belong to
    struct LinkStage {
        DevBuf ptr, bits, cnt, off, ctr, part, out;
        EventTimer t_total;
        elba_graph_stats stats{};
        uint64_t for_cg = 0;
        void release_scratch() { for (DevBuf *b : {&ptr, &bits, &cnt, &off, &ctr, &part, &out}) b->release(); }
    } gl;

    // read pileups (pileup.hip): results (depth.seg_off, depth.seg_start, depth.seg_depth, trim, flags) and the counters survive
    // elba_release_workspace, the rest is scratch
    struct PileupStage {
        int64_t M = 0, n = 0, nseg = 0;
        DepthBufs depth;
        DevBuf ctr, sel, rows, cols, vals;
        DevBuf trim, flags;
        EventTimer t_total;
        elba_pileup_stats stats{};
        elba_pileup_cfg cfg{};                  // the cfg of the pileup that is valid now (trim.hip's long runs are its min_depth / min_run)
        void release_scratch() { depth.release_scratch(); for (DevBuf *b : {&sel, &rows, &cols, &vals}) b->release(); }
    } pu;

    // read placements and contig depth (place.hip): all scratch, in buffers of its own so that a valid pileup stays untouched — chain start /
    // strand per read, the winning candidate per read, the records, contig lengths, the endpoint keys and what the pileup's keys-to-segments
    // sequence needs (depth), per-contig credits, the counters.  for_cg: the contig call (cg.serial) the counts in stats belong to
    struct PlaceStage {
        DevBuf cstart, cstrand, best, rec, clen, cred, ctr;
        DepthBufs depth;
        EventTimer t_total;
        elba_place_stats stats{};
        uint64_t for_cg = 0;
        void release_scratch() { for (DevBuf *b : {&cstart, &cstrand, &best, &rec, &clen, &cred, &ctr}) b->release(); depth.release(); }
    } pl;

    // contig polishing (polish.hip): all scratch — per read its slice (rows, first column, first base) and record, the row offsets of the
    // choices, the choices of one batch, the votes (5 per column, 4 per gap), what every column emits and its scan, the per-contig counts,
    // the polished bases.  for_cg: the contig call (cg.serial) the counts in stats belong to
    struct PolishStage {
        DevBuf plan, rec, toff, trace, col, gap, cnt, emit, off, cstat, seq, seqoff, ctr;
        EventTimer t_total;
        elba_polish_stats stats{};
        uint64_t for_cg = 0;
        void release_scratch() { for (DevBuf *b : {&plan, &rec, &toff, &trace, &col, &gap, &cnt, &emit, &off, &cstat, &seq, &seqoff, &ctr}) b->release(); }
    } po;

    // trimmed reads (trim.hip): a snapshot in buffers of its own — packed / off / len in DnaBuffer layout, the map (src, beg, end); it survives
    // elba_prune_reads and elba_release_workspace (as do the counters), a new read set or a new pileup invalidates it, elba_adopt_trimmed_reads consumes it
    struct TrimStage {
        int64_t n = 0, packed_bytes = 0;
        DevBuf packed, off, len, src, beg, end, ctr;
        DevBuf cnt, bytes, first, boff, srcb;      // scratch
        EventTimer t_total, t_repack;
        elba_trim_stats stats{};
        void release_scratch() { for (DevBuf *b : {&cnt, &bytes, &first, &boff, &srcb}) b->release(); }
    } tm;

    // string graph cleaning (sg_rounds.hpp): what the five calls below share, all scratch.  Column pointers of the round's S, the removed reads,
    // keep flags and their scan, the counters, and the second buffer of S (rows, cols, vals: swapped with tr_out_* after an odd number of
    // moves).  The calls run one after another on the context's stream and each reads its two times before it returns: one pair of timers
    struct SgWork {
        DevBuf ptr, removed, keep, pos, st, rows, cols, vals;
        EventTimer t_total, t_compact;
        void release() { ptr.release(); removed.release(); keep.release(); pos.release(); st.release(); rows.release(); cols.release(); vals.release(); }
    } sg;

    // tip clipping (tips.hip): scratch of its own, one word per read each
    struct TipStage { DevBuf ntips, anchor; elba_tip_stats stats{}; void release_scratch() { ntips.release(); anchor.release(); } } tp;

    // bubble popping (bubbles.hip): scratch of its own, one word per entry of S each
    struct BubbleStage { DevBuf end, len; elba_bubble_stats stats{}; void release_scratch() { end.release(); len.release(); } } bb;

    // cutting weak overlaps (weak.hip): scratch of its own, one word per (read, side) each
    struct WeakStage { DevBuf best, cnt, nweak, after; elba_weak_stats stats{}; void release_scratch() { best.release(); cnt.release(); nweak.release(); after.release(); } } wk;

    // cutting bridge chains (bridges.hip): scratch of its own, one word per entry of S
    struct BridgeStage { DevBuf flank; elba_bridge_stats stats{}; void release_scratch() { flank.release(); } } br;

    // resolving three-armed stars (stars.hip): scratch of its own, one word per read.  It reads tr_ptr / tr_sym
    struct StarStage { DevBuf word; elba_star_stats stats{}; void release_scratch() { word.release(); } } sr;

    // connected components (components.hip): all scratch — the label of every read, degrees, the column pointers of S, root flags and their
    // scan, the component of every read, the counters, the six tables of M slots each, and the partition's two arrays.  graph: the kind the
    // counts in stats belong to (-1: none)
    struct ComponentStage {
        DevBuf par, deg, ptr, flag, rank, comp, st, tab, pcomp, pread;
        EventTimer t_total, t_label;
        elba_cc_stats stats{};
        int graph = -1;
        void release_scratch() { for (DevBuf *b : {&par, &deg, &ptr, &flag, &rank, &comp, &st, &tab, &pcomp, &pread}) b->release(); }
    } cc;

    // the induced sub-problem of one part (induce.hip): results — old_of_new, the part's reads in DnaBuffer layout (packed / off / len), its
    // pairs (rows / cols / vals) and the outside counters (oa / op) — are what elba_induced_t's device views point at; they and the scratch
    // (the selection and its scans, new_of_old, source base offsets, keep flags and their scan, part_of_read, the counters) go with
    // elba_release_workspace: the views are valid until then
    struct InduceStage {
        DevBuf old_of_new, packed, off, len, rows, cols, vals, oa, op;
        DevBuf part, sel, bytes, first, boff, new_of_old, srcb, keep, pos, ctr;      // scratch
        EventTimer t_total, t_pairs, t_scatter, t_gather;      // (the pairs' time is t_pairs + t_scatter: the first synchronisation lies between them)
        elba_induce_stats stats{};
        void release_scratch()
        {
            for (DevBuf *b : {&old_of_new, &packed, &off, &len, &rows, &cols, &vals, &oa, &op, &part, &sel, &bytes, &first, &boff, &new_of_old, &srcb, &keep, &pos, &ctr}) b->release();
        }
    } in;

    // workspaces
    DevBuf ws_scan, ws_sort, ws_a, ws_b, ws_c, ws_d, ws_e, ws_f;
    DevBuf ws_cursor;       // the gather-slot cursor of the k-mer stage's emit kernels (kmer_msd.hip)
    DevBuf ws_g, ws_h;      // crowded buckets of the wide k-mer partition (kmer_msd.hip: k31_gather_crowded ...): their records / the pseudo-buckets' arrays
    DevBuf ov_totcnt, ov_mir, ov_tmp, ov_sum_tmp;  // u32[M+1] mirrored entries per row (ticket counters); mirrored entries laid out like B (32-byte records); staging area (32-byte records)
    bool ov_low_clean = false;                 // the ticket counters are all zero (handed back clean by the previous call)
    DevBuf ov_rowcnt, ov_rowoff, ov_lists, ov_counters, ov_gtable, ov_sortkeys;
    int64_t ov_tmp_cap = 0;
    bool ov_sort_used[2] = {false, false};      // wide-row sorts used by the previous call
    bool ov_tiers_known = false, ov_tier_used[8] = {false, false, false, false, false, false, false, false};   // tiers that got rows in the previous call
    int64_t b_cap_entries = 0;      // capacity of b_col/b_val the next overlap call may assume (0 = unknown: size it after the numeric pass)
    uint64_t ov_calls = 0;          // steady-state overlap calls so far (phase events are recorded on every cfg.timing_stride-th)
    uint32_t ov_prior_q16 = 0;      // distinct-partner / product ratio measured by the previous overlap call (x 65536), 0 = unknown
    uint32_t ov_slab_q16 = 0;       // mirrored entries per row entry of A measured by the previous call on the whole matrix (x 65536, without the margin), 0 = unknown
    DevBuf ov_slab;                 // uint4[ov_slab_cap]: the rows' mirror slabs (spgemm.hip)
    int64_t ov_slab_cap = 0;
    DevBuf ov_tickrows;             // u32[M / 32 + 1]: rows that staged an entry whose image took a ticket (spgemm.hip: OvParams::tick_rows)
    DevBuf ov_slabpos, ov_slabn;    // u64[M] slab end << 32 | next free entry; u32[M] entries in every row's slab (spgemm.hip)
    bool ov_slab_on = false;        // the running call has slabs (ov_launch_finalize reads them)
    uint32_t ov_slab_q16_used = 0;  // diagnostic: the ratio the last call's slabs were sized by (margin included), 0 = none
    int64_t ov_mir_placed = 0;      // diagnostic: mirrored entries of the last call that did NOT go to a slab (placed by k_mirror)
    int64_t ov_spec_geom = 0;       // diagnostic: ... and they were its compiled-geometry variant (ov_plan.hpp: ov_spec_geom_ok)
    int64_t ov_spec = 0;            // diagnostic: the last call's numeric kernels were the reads-path instantiation (1) or the general one (0)
    // diagnostics of the last create_seed_matrix, from its final pass (elba_get_stat "overlap_tier_*", "overlap_sort_rows_*", "overlap_family", "overlap_pay16",
    // "overlap_rec16"): the plan's claim limits, the rows queued / completed per tier, the rows the two wide-row sorts took, the kernel family and record format
    int64_t ov_tier_limit[5] = {0, 0, 0, 0, 0}, ov_tier_queued[6] = {0, 0, 0, 0, 0, 0}, ov_tier_done[6] = {0, 0, 0, 0, 0, 0}, ov_sort_rows[2] = {0, 0};
    int64_t ov_family = 0, ov_pay16 = 0, ov_rec16_used = 0;
    int64_t ov_passes = 0, ov_forwarded = 0;      // diagnostic: passes the last call took (1 = no repeat); rows its numeric kernels forwarded on a prediction (spgemm_direct.hpp)
    // sharded call with mirror exchange (spgemm.hip: stage_seed_matrix_begin / _fill / _end)
    int ov_phase = 0;               // 1: begin has run (numeric done, staged records waiting), end not yet
    int ov_pend_passes = 1; bool ov_pend_timed = false; float ov_pend_ms[3] = {0, 0, 0};
    std::vector<uint64_t> ov_remote_bounds;
    DevBuf ov_remote;               // mirror images received from other ranks (32-byte records)
    int64_t ov_send_slot = 0;       // slot size of the step in flight (stage_seed_matrix_send): recv must be given the same
    DevBuf ov_cursors;              // per-destination cursors of the fixed-slot exchange + the receive side's check words (stage_seed_matrix_send / _recv)
    bool own_stream = true;         // c.stream was created by the context (elba_set_stream: the caller's)

    EventTimer t_total, t_a, t_b, t_c;
    EventTimer t_emit, t_emit_plain; int64_t prep_us = -1, emit_us = -1;      // Options::measure_prep
    struct PinnedHost { void *p = nullptr; size_t cap = 0; void reserve(size_t n) { if (n <= cap) return; if (p) (void)hipHostFree(p); p = nullptr; cap = 0; ELBA_HIP(hipHostMalloc(&p, n, hipHostMallocDefault)); cap = n; } ~PinnedHost() { if (p) (void)hipHostFree(p); } };
    PinnedHost ov_host;            // pinned landing area of the per-call counter read-back (a pageable target makes the copy a staged, blocking one)
    PhaseMarks<5> ov_marks;        // overlap SpGEMM: 0 call start, 1 numeric start, 2 numeric end, 3 call end, 4 finalize start when the host synchronised before it
};

// a new read set is in place (elba_set_reads*, elba_adopt_trimmed_reads): ev's row, and an A built from the old reads goes with them
inline void reads_replaced(Ctx &c, Event ev)
{
    done(c.v, ev);
    if (c.A_has_kmers) done(c.v, EV_MATRIX_OF_OLD_READS);
    c.tx_index = false;      // (elba_set_reads_text sets it again behind this call)
    c.tr_outside = false;    // (the loaded edge list went with the old reads, and its outside counts with it)
}

// The pairs the string graph is built from — what elba_transitive_reduction, elba_read_pileup and elba_prune_reads read: a loaded edge
// list while one is valid, else this context's own alignments of a whole B.  id_base: what the exported graph adds to its read ids.
struct GraphInput { int64_t M, n, id_base; const int64_t *rows, *cols; const elba_overlap_t *vals; };
inline GraphInput graph_input(Ctx &c, const char *who)
{
    if (has(c.v, P_EDGES)) return {c.tr_in_M, c.tr_in_n, 0, c.tr_in_rows.as<int64_t>(), c.tr_in_cols.as<int64_t>(), c.tr_in_vals.as<elba_overlap_t>()};
    ELBA_REQUIRE(has(c.v, P_ALN), ELBA_ERR_STATE, std::string(who) + ": no overlaps (call elba_align_seeds or elba_set_overlaps)");
    ELBA_REQUIRE(c.row_hi < 0 || (c.row_lo == 0 && c.row_hi == c.M), ELBA_ERR_STATE,
                 std::string(who) + ": this context aligned a row shard; gather the ranks' overlaps and load them with elba_set_overlaps");
    return {c.M, c.naln, c.first_global_id_rows(), c.aln_rows.as<int64_t>(), c.aln_cols.as<int64_t>(), c.aln_out.as<elba_overlap_t>()};
}

// Where reads 0 .. M-1 are: the replicated set (elba_dist_set_all_reads) when it holds M reads and the caller takes it, else the context's
// own.  what: the reads as the error names them, '#' standing for M.
struct ReadSource { const uint8_t *packed; const uint64_t *byte_off; const uint32_t *len; bool replicated; };
inline ReadSource read_source(Ctx &c, int64_t M, const char *who, const char *what, bool take_replicated = true)
{
    if (take_replicated && c.aln_all_n == M && c.aln_all_n >= 0) return {c.aln_all_packed.as<uint8_t>(), c.aln_all_off.as<uint64_t>(), c.aln_all_len.as<uint32_t>(), true};
    if (has(c.v, P_READS) && c.nreads == M) return {c.d_packed, c.d_byte_off, c.d_len, false};
    std::string w(what);
    w.replace(w.find('#'), 1, std::to_string(M));
    throw Error{ELBA_ERR_STATE, std::string(who) + ": the " + w + " are not on this context (elba_set_reads or elba_dist_set_all_reads)"};
}

const uint64_t *depth_segments(Ctx &c, DepthBufs &b, int64_t E, int64_t M, int mb, int pb, const uint32_t *len, unsigned long long *ctr);      // pileup.hip

// What an export hands to the caller: a malloc'ed block of at least one element (the elba_free_* functions free it), and the copy of n
// elements from the device into it, queued on the context's stream
template <class T>
T *host_block(size_t n)
{
    T *p = static_cast<T *>(malloc((n ? n : 1) * sizeof(T)));
    if (!p) throw std::bad_alloc();
    return p;
}
template <class T>
void copy_out(Ctx &c, T *dst, const void *src, size_t n)
{
    if (n) ELBA_HIP(hipMemcpyAsync(dst, src, n * sizeof(T), hipMemcpyDeviceToHost, c.stream));
}

// pair a of the graph's input has a bad interval (the smallest such pair, found by a kernel of read_pileup, place_reads or polish_contigs)
[[noreturn]] void throw_bad_pair(Ctx &c, const GraphInput &in, int64_t a, const char *who);      // pileup.hip

// elba_place_reads up to and including its records (place.hip), for the two stages that need them: the state and size checks (messages
// begin with `who`), the reservations, chain starts, the candidates' winners and k_pl_place — queued on the context's stream, not
// synchronised.  ctr: the PLACE_CTR_WORDS counters of place.hip; word PLACE_CTR_BAD holds the smallest candidate with a bad interval (all
// ones: none), which the caller reads behind its own synchronisation and hands to throw_bad_pair.  depth_bufs: also reserve what
// depth_segments needs.  t, when given, is started in front of the first launch.
constexpr int PLACE_CTR_BAD = 2, PLACE_CTR_WORDS = 16;
struct PlaceWork { GraphInput in; ReadSource src; int64_t M, base, E, nc; elba_placement_t *rec; unsigned long long *ctr; const uint32_t *clen; };
PlaceWork place_records(Ctx &c, int skip_flags, const char *who, bool depth_bufs, EventTimer *t);

// ---- stages -----------------------------------------------------------------------------------------------------
void stage_set_reads_fasta(Ctx &c, const char *chunk, int64_t chunk_bytes, uint64_t chunk_file_offset, const elba_fasta_record_t *recs, int64_t nreads,
                           int64_t first_global_id, elba_ingest_stats *stats);      // ingest.hip
void launch_fasta_encode(Ctx &c, const uint8_t *d_chunk, uint64_t chunk_file_offset, uint64_t chunk_bytes, const elba_fasta_record_t *d_recs, const uint64_t *d_byte_off,
                         int64_t nreads, uint8_t *d_packed);      // ingest.hip: k_fasta_encode on records that are on the device already (nreads > 0)
constexpr uint32_t TEXT_TILE_BYTES = 4096;                        // text_index.hip: bytes of the chunk one workgroup takes per trip (elba_get_stat "text_tile_bytes")
void stage_set_reads_text(Ctx &c, const char *chunk, int64_t chunk_bytes, uint64_t chunk_file_offset, const elba_text_cfg *cfg, elba_text_stats *stats);      // text_index.hip
void stage_export_read_index(Ctx &c, elba_fasta_record_t *recs, uint64_t *name_pos, uint32_t *name_len, int64_t nreads_capacity);
void stage_count_kmers(Ctx &c);                                   // kmer.hip
void stage_create_kmer_matrix(Ctx &c);                            // kmer.hip
bool msd_matrix_from_triples(Ctx &c, int64_t M, int64_t N, int64_t Z, const int64_t *d_rows, const int64_t *d_cols, const uint32_t *d_vals);   // kmer_msd.hip: false = matrix.hip sorts
bool msd_count_kmers(Ctx &c, uint64_t I, elba_kmer_stats &st);   // kmer_msd.hip: false = not applicable (the caller sorts)
void choose_column_store(Ctx &c, int64_t N, int64_t max_col);     // matrix.hip: padded column store or plain CSC, strides, sequence-number bits
inline CsrOptions csr_options(const Ctx &c)                       // the options csr_plan.hpp's decisions read
{
    CsrOptions o;
    o.csr_pairs = c.opt.csr_pairs; o.no_hints = c.opt.no_hints; o.no_pay = c.opt.no_pay; o.no_inline = c.opt.no_inline; o.no_symmetry = c.opt.no_symmetry; o.no_ell = c.opt.no_ell;
    o.no_suffix = c.opt.no_suffix; o.panel_inline = c.opt.panel_inline; o.no_row_order = c.opt.no_row_order; o.tune1 = c.opt.tune[1];
    return o;
}
void stage_set_kmer_matrix(Ctx &c, int64_t M, int64_t N, int64_t Z, const int64_t *rows, const int64_t *cols, const uint32_t *vals);  // matrix.hip
void stage_set_kmer_matrix_device(Ctx &c, int64_t M, int64_t N, int64_t Z, const int64_t *d_rows, const int64_t *d_cols, const uint32_t *d_vals);
void stage_export_triples_device(Ctx &c, int64_t *d_rows, int64_t *d_cols, uint32_t *d_vals);
void stage_create_seed_matrix(Ctx &c);                            // spgemm.hip
void stage_seed_matrix_begin(Ctx &c, int nranks, const uint64_t *bounds_host, uint64_t *send_counts_host);
void stage_seed_matrix_fill(Ctx &c, void *d_send, const uint64_t *offsets_host);
void stage_seed_matrix_end(Ctx &c, const void *d_recv, int64_t nrecv);
void stage_seed_matrix_send(Ctx &c, int nranks, const uint64_t *bounds_host, void *d_send, int64_t slot);
bool stage_seed_matrix_recv(Ctx &c, void *d_recv, int64_t slot, int64_t *slot_needed);
void stage_align_seeds(Ctx &c, int mat, int mis, int gap, int dropoff);   // align.hip
void stage_dist_set_all_reads(Ctx &c, const void *d_packed, int64_t packed_bytes, const void *d_byte_off, const void *d_len, int64_t nreads_total);   // align.hip
void stage_set_overlaps(Ctx &c, int64_t nreads, const int64_t *rows, const int64_t *cols, const elba_overlap_t *vals, int64_t n);   // tr.hip
void stage_set_overlaps_device(Ctx &c, int64_t nreads, const void *d_rows, const void *d_cols, const void *d_vals, int64_t n);
void stage_set_outside_counts(Ctx &c, int64_t nreads, const void *aligned, const void *passed, bool on_device);
void stage_transitive_reduction(Ctx &c, double bad_read_cutoff, int fuzz);   // tr.hip
void stage_generate_contigs(Ctx &c, int flags);                                          // contig.hip
void stage_generate_contigs_ex(Ctx &c, const elba_contig_cfg *cfg);                      // contig.hip
void stage_export_assembly_links(Ctx &c, elba_links_t *out);                             // graph_links.hip (out->links: malloc)
void stage_place_reads(Ctx &c, const elba_place_cfg *cfg, elba_placements_t *out);        // place.hip (out's arrays: malloc)
void stage_polish_contigs(Ctx &c, const elba_polish_cfg *cfg, elba_polished_t *out);       // polish.hip (out's arrays: malloc)
void stage_graph_components(Ctx &c, const elba_cc_cfg *cfg, elba_components_t *out);      // components.hip (out's arrays: malloc)
void stage_partition_components(Ctx &c, const elba_part_cfg *cfg, int32_t *part_of_read, int64_t nreads, int64_t *part_weight);
void stage_induce_part(Ctx &c, const elba_induce_cfg *cfg, const int32_t *part_of_read, int64_t nreads, elba_induced_t *out);      // induce.hip (out's host arrays: malloc)
void stage_read_pileup(Ctx &c, const elba_pileup_cfg *cfg);                   // pileup.hip
void stage_prune_reads(Ctx &c, int mask, int64_t *kept);
void stage_trim_reads(Ctx &c, const elba_trim_cfg *cfg);                      // trim.hip
void stage_adopt_trimmed_reads(Ctx &c);
void stage_clip_tips(Ctx &c, const elba_tip_cfg *cfg);                        // tips.hip
void stage_pop_bubbles(Ctx &c, const elba_bubble_cfg *cfg);                   // bubbles.hip
void stage_cut_weak_overlaps(Ctx &c, const elba_weak_cfg *cfg);              // weak.hip
void stage_cut_bridges(Ctx &c, const elba_bridge_cfg *cfg);                   // bridges.hip
void stage_resolve_stars(Ctx &c, const elba_star_cfg *cfg);                   // stars.hip
void stage_dist_count_owners(Ctx &c, int nranks, uint64_t *counts_host);                                   // kmer.hip
void stage_dist_value_histogram(Ctx &c, uint64_t *hist_host, int64_t nbins);
void stage_ref_hash_owner(Ctx &c, const uint64_t *kmers_host, int64_t n, int nprocs, uint64_t *hash_host, int32_t *owner_host);
void stage_dist_set_owner_ranges(Ctx &c, int nranks, const uint32_t *upper_bins);
void stage_dist_set_kmer_id_base(Ctx &c, int64_t base, int64_t nall);
void stage_dist_fill_send(Ctx &c, int nranks, void *d_send, const uint64_t *offsets_host);
bool stage_dist_packed_format(Ctx &c, int nranks, const int64_t *bounds, const uint32_t *all_lens, int *value_bits, int *index_bits);
void stage_dist_fill_send_packed(Ctx &c, int nranks, void *d_send, const uint64_t *offsets_host);
void stage_dist_unpack_records(Ctx &c, int nranks, int rank, const void *d_packed, const uint64_t *recv_counts_host, void *d_out);
void stage_dist_count_records(Ctx &c, const void *d_rec, int64_t nrec);
void stage_dist_copy_reliable_kmers(Ctx &c, void *d_dst);       // N k-mers of 1 + (k > 32) + (k > 64) words each, interleaved
void stage_dist_set_global_kmers(Ctx &c, const void *d_all, int64_t nall);
void stage_dist_panel(Ctx &c, int nranks, const uint64_t *bounds_host, const uint64_t *win_lo_host, const uint64_t *win_hi_host, bool fill, void *d_send, uint64_t *counts_or_offsets_host);
void stage_dist_set_panel(Ctx &c, const void *d_rec, int64_t nrec, int64_t M_total, int64_t N_total, int64_t row_lo, int64_t row_hi);

}  // namespace elba
