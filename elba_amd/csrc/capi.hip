// capi.hip — the extern "C" surface declared in include/elba_amd.h.  Every entry point converts elba::Error into a status
// code + elba_last_error text; nothing here computes on the CPU except index bookkeeping of exported copies.
#include "common.hpp"
#include "ov_plan.hpp"
#include <new>

using namespace elba;

struct elba_ctx {
    Ctx c;
};

namespace {

template <class F>
int guarded(elba_ctx *ctx, F &&f)
{
    if (!ctx) return ELBA_ERR_INVALID_ARG;
    try {
        ELBA_HIP(hipSetDevice(ctx->c.device));
        f(ctx->c);
        return ELBA_OK;
    } catch (const Error &e) {
        ctx->c.last_error = e.msg;
        return e.code;
    } catch (const std::bad_alloc &) {
        ctx->c.last_error = "host allocation failed";
        return ELBA_ERR_OUT_OF_MEMORY;
    } catch (...) {
        ctx->c.last_error = "unknown exception";
        return ELBA_ERR_INTERNAL;
    }
}

// elba_get_stat's counters of one late stage: the names behind the stage's prefix and where each stands in its stats struct
template <class S> struct StatName { const char *name; int64_t S::*field; };
template <class S, size_t N>
int64_t stage_stat(const StatName<S> (&table)[N], const S &st, bool valid, const char *field, const char *name)
{
    for (const StatName<S> &e : table) if (!strcmp(field, e.name)) return valid ? st.*e.field : 0;
    throw Error{ELBA_ERR_INVALID_ARG, std::string("get_stat: unknown counter ") + name};
}

template <class T>
std::vector<T> download(Ctx &c, const void *d, size_t n)
{
    std::vector<T> h(n);
    if (n) ELBA_HIP(hipMemcpyAsync(h.data(), d, n * sizeof(T), hipMemcpyDeviceToHost, c.stream));
    ELBA_HIP(hipStreamSynchronize(c.stream));
    return h;
}

}  // namespace

extern "C" {

int elba_abi_version(void) { return ELBA_ABI_VERSION; }

const char *elba_strerror(int status)
{
    switch (status) {
    case ELBA_OK: return "ok";
    case ELBA_ERR_INVALID_ARG: return "invalid argument";
    case ELBA_ERR_NO_DEVICE: return "no HIP device available (this library has no CPU fallback)";
    case ELBA_ERR_HIP: return "HIP runtime error";
    case ELBA_ERR_OUT_OF_MEMORY: return "out of memory";
    case ELBA_ERR_STATE: return "stage called out of order";
    case ELBA_ERR_UNSUPPORTED: return "unsupported configuration";
    case ELBA_ERR_INTERNAL: return "internal error";
    case ELBA_ERR_RETRY: return "some rank ran out of room: repeat the step";
    default: return "unknown status";
    }
}

const char *elba_last_error(const elba_ctx *ctx) { return ctx ? ctx->c.last_error.c_str() : "null context"; }

int elba_ctx_create(elba_ctx **out, const elba_cfg *cfg)
{
    if (!out || !cfg) return ELBA_ERR_INVALID_ARG;
    *out = nullptr;
    // include/compiletime.h:10,21: k odd, 2 < k < 96, 0 < L <= U <= 65535.  Here: one 64-bit word per k-mer (k <= 31).
    if (cfg->k < 3 || !(cfg->k & 1) || cfg->k >= 96) return ELBA_ERR_INVALID_ARG;
    if (cfg->lower < 1 || cfg->lower > cfg->upper || cfg->upper > 65535) return ELBA_ERR_INVALID_ARG;
    /* 3 <= k <= 95, odd: the reference's range (include/compiletime.h:10); one, two or three words per k-mer */
    if (cfg->lower < 2) return ELBA_ERR_UNSUPPORTED;   // LOWER == 1 is nondeterministic in the reference
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return ELBA_ERR_NO_DEVICE;
    if (cfg->device < 0 || cfg->device >= ndev) return ELBA_ERR_INVALID_ARG;
    elba_ctx *ctx = new (std::nothrow) elba_ctx();
    if (!ctx) return ELBA_ERR_OUT_OF_MEMORY;
    ctx->c.cfg = *cfg;
    ctx->c.device = cfg->device;
    int rc = guarded(ctx, [&](Ctx &c) {
        ELBA_HIP(hipStreamCreateWithFlags(&c.stream, hipStreamNonBlocking));
        hipDeviceProp_t prop;
        ELBA_HIP(hipGetDeviceProperties(&prop, c.device));
        c.num_cus = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    });
    if (rc != ELBA_OK) { delete ctx; return rc; }
    *out = ctx;
    return ELBA_OK;
}

void elba_ctx_destroy(elba_ctx *ctx)
{
    if (!ctx) return;
    (void)hipSetDevice(ctx->c.device);
    if (ctx->c.stream) { (void)hipStreamSynchronize(ctx->c.stream); if (ctx->c.own_stream) (void)hipStreamDestroy(ctx->c.stream); }
    delete ctx;
}

static void check_reads_host(const uint64_t *byte_off, const uint32_t *len, int64_t nreads, int64_t *packed_bytes)
{
    int64_t end = 0;
    for (int64_t r = 0; r < nreads; ++r) {
        int64_t e = (int64_t)byte_off[r] + ((int64_t)len[r] + 3) / 4;
        if (e > end) end = e;
    }
    *packed_bytes = end;
}

int elba_set_reads(elba_ctx *ctx, const uint8_t *packed, const uint64_t *byte_off, const uint32_t *len, int64_t nreads, int64_t first_global_id)
{
    return guarded(ctx, [&](Ctx &c) {
        enter(c.v, EV_SET_READS);
        ELBA_REQUIRE(nreads >= 0 && (nreads == 0 || (packed && byte_off && len)), ELBA_ERR_INVALID_ARG, "set_reads: null array");
        ELBA_REQUIRE(nreads < 0xFFFFFFFFll, ELBA_ERR_UNSUPPORTED, "set_reads: more than 2^32-1 reads on one GPU");
        accepted(c.v, EV_SET_READS);
        int64_t pb = 0;
        check_reads_host(byte_off, len, nreads, &pb);
        c.own_packed.reserve((size_t)pb + 16);       // +16: the enumerate kernel reads whole 8-byte windows
        c.own_byte_off.reserve((size_t)(nreads + 1) * 8);
        c.own_len.reserve((size_t)(nreads + 1) * 4);
        ELBA_HIP(hipMemsetAsync(c.own_packed.p, 0, (size_t)pb + 16, c.stream));
        if (pb) ELBA_HIP(hipMemcpyAsync(c.own_packed.p, packed, (size_t)pb, hipMemcpyHostToDevice, c.stream));
        if (nreads) {
            ELBA_HIP(hipMemcpyAsync(c.own_byte_off.p, byte_off, (size_t)nreads * 8, hipMemcpyHostToDevice, c.stream));
            ELBA_HIP(hipMemcpyAsync(c.own_len.p, len, (size_t)nreads * 4, hipMemcpyHostToDevice, c.stream));
        }
        ELBA_HIP(hipStreamSynchronize(c.stream));
        c.d_packed = c.own_packed.as<uint8_t>(); c.d_byte_off = c.own_byte_off.as<uint64_t>(); c.d_len = c.own_len.as<uint32_t>();
        c.h_len.assign(len, len + nreads);
        c.h_byte_off.assign(byte_off, byte_off + nreads);
        c.nreads = nreads; c.first_global_id = first_global_id; c.packed_bytes = pb;
        reads_replaced(c, EV_SET_READS);
    });
}

int elba_set_reads_fasta(elba_ctx *ctx, const char *chunk, int64_t chunk_bytes, uint64_t chunk_file_offset, const elba_fasta_record_t *recs, int64_t nreads,
                         int64_t first_global_id, elba_ingest_stats *stats)
{
    return guarded(ctx, [&](Ctx &c) { stage_set_reads_fasta(c, chunk, chunk_bytes, chunk_file_offset, recs, nreads, first_global_id, stats); });
}

int elba_set_reads_text(elba_ctx *ctx, const char *chunk, int64_t chunk_bytes, uint64_t chunk_file_offset, const elba_text_cfg *cfg, elba_text_stats *stats)
{
    return guarded(ctx, [&](Ctx &c) { stage_set_reads_text(c, chunk, chunk_bytes, chunk_file_offset, cfg, stats); });
}

int elba_export_read_index(elba_ctx *ctx, elba_fasta_record_t *recs, uint64_t *name_pos, uint32_t *name_len, int64_t nreads_capacity)
{
    return guarded(ctx, [&](Ctx &c) { stage_export_read_index(c, recs, name_pos, name_len, nreads_capacity); });
}

int elba_export_reads(elba_ctx *ctx, uint8_t *packed, int64_t packed_capacity, uint64_t *byte_off, uint32_t *len, int64_t nreads_capacity)
{
    return guarded(ctx, [&](Ctx &c) {
        ELBA_REQUIRE(has(c.v, P_READS), ELBA_ERR_STATE, "export_reads: no reads");
        if (packed) {
            ELBA_REQUIRE(packed_capacity >= c.packed_bytes, ELBA_ERR_INVALID_ARG, "export_reads: packed buffer too small");
            if (c.packed_bytes) ELBA_HIP(hipMemcpyAsync(packed, c.d_packed, (size_t)c.packed_bytes, hipMemcpyDeviceToHost, c.stream));
        }
        if (byte_off || len) ELBA_REQUIRE(nreads_capacity >= c.nreads, ELBA_ERR_INVALID_ARG, "export_reads: offset/length arrays too small");
        if (byte_off && c.nreads) ELBA_HIP(hipMemcpyAsync(byte_off, c.d_byte_off, (size_t)c.nreads * 8, hipMemcpyDeviceToHost, c.stream));
        if (len && c.nreads) ELBA_HIP(hipMemcpyAsync(len, c.d_len, (size_t)c.nreads * 4, hipMemcpyDeviceToHost, c.stream));
        ELBA_HIP(hipStreamSynchronize(c.stream));
    });
}

int elba_set_reads_device(elba_ctx *ctx, const void *d_packed, int64_t packed_bytes, const void *d_byte_off, const void *d_len, int64_t nreads, int64_t first_global_id)
{
    return guarded(ctx, [&](Ctx &c) {
        enter(c.v, EV_SET_READS_DEVICE);
        ELBA_REQUIRE(nreads >= 0 && packed_bytes >= 0 && (nreads == 0 || (d_packed && d_byte_off && d_len)), ELBA_ERR_INVALID_ARG, "set_reads_device: null array");
        ELBA_REQUIRE(nreads < 0xFFFFFFFFll, ELBA_ERR_UNSUPPORTED, "set_reads_device: more than 2^32-1 reads on one GPU");
        accepted(c.v, EV_SET_READS_DEVICE);
        // the packed buffer is copied once device-to-device so that the 16 guard bytes behind it exist; offsets/lengths are borrowed
        c.own_packed.reserve((size_t)packed_bytes + 16);
        ELBA_HIP(hipMemsetAsync(c.own_packed.p, 0, (size_t)packed_bytes + 16, c.stream));
        if (packed_bytes) ELBA_HIP(hipMemcpyAsync(c.own_packed.p, d_packed, (size_t)packed_bytes, hipMemcpyDeviceToDevice, c.stream));
        c.d_packed = c.own_packed.as<uint8_t>();
        c.d_byte_off = static_cast<const uint64_t *>(d_byte_off);
        c.d_len = static_cast<const uint32_t *>(d_len);
        c.h_len = download<uint32_t>(c, d_len, (size_t)nreads);
        c.h_byte_off = download<uint64_t>(c, d_byte_off, (size_t)nreads);
        for (int64_t r = 0; r < nreads; ++r)
            ELBA_REQUIRE((int64_t)c.h_byte_off[r] + ((int64_t)c.h_len[r] + 3) / 4 <= packed_bytes, ELBA_ERR_INVALID_ARG, "set_reads_device: read exceeds the packed buffer");
        c.nreads = nreads; c.first_global_id = first_global_id; c.packed_bytes = packed_bytes;
        reads_replaced(c, EV_SET_READS_DEVICE);
    });
}

int elba_count_kmers(elba_ctx *ctx, elba_kmer_stats *stats)
{
    return guarded(ctx, [&](Ctx &c) {
        stage_count_kmers(c);
        if (stats) *stats = c.kstats;
    });
}

int elba_create_kmer_matrix(elba_ctx *ctx, elba_matrix_stats *stats)
{
    return guarded(ctx, [&](Ctx &c) {
        EventTimer t;
        t.start(c.stream);
        stage_create_kmer_matrix(c);
        t.stop(c.stream);
        if (stats) { stats->nrows = c.M; stats->ncols = c.N; stats->nnz = c.Z; stats->max_row_nnz = c.max_row_nnz; stats->ms_total = t.ms(); }
    });
}

int elba_set_kmer_matrix(elba_ctx *ctx, int64_t nrows, int64_t ncols, int64_t nnz, const int64_t *rows, const int64_t *cols, const uint32_t *vals, elba_matrix_stats *stats)
{
    return guarded(ctx, [&](Ctx &c) {
        EventTimer t;
        t.start(c.stream);
        stage_set_kmer_matrix(c, nrows, ncols, nnz, rows, cols, vals);
        t.stop(c.stream);
        if (stats) { stats->nrows = c.M; stats->ncols = c.N; stats->nnz = c.Z; stats->max_row_nnz = c.max_row_nnz; stats->ms_total = t.ms(); }
    });
}

int elba_set_kmer_matrix_device(elba_ctx *ctx, int64_t nrows, int64_t ncols, int64_t nnz, const void *d_rows, const void *d_cols, const void *d_vals, elba_matrix_stats *stats)
{
    return guarded(ctx, [&](Ctx &c) {
        EventTimer t;
        t.start(c.stream);
        stage_set_kmer_matrix_device(c, nrows, ncols, nnz, static_cast<const int64_t *>(d_rows), static_cast<const int64_t *>(d_cols), static_cast<const uint32_t *>(d_vals));
        t.stop(c.stream);
        if (stats) { stats->nrows = c.M; stats->ncols = c.N; stats->nnz = c.Z; stats->max_row_nnz = c.max_row_nnz; stats->ms_total = t.ms(); }
    });
}

int elba_export_triples_device(elba_ctx *ctx, void *d_rows, void *d_cols, void *d_vals)
{
    return guarded(ctx, [&](Ctx &c) { stage_export_triples_device(c, static_cast<int64_t *>(d_rows), static_cast<int64_t *>(d_cols), static_cast<uint32_t *>(d_vals)); });
}

int elba_create_seed_matrix(elba_ctx *ctx, elba_overlap_stats *stats)
{
    return guarded(ctx, [&](Ctx &c) {
        stage_create_seed_matrix(c);
        if (stats) *stats = c.ostats;
    });
}

int elba_seed_matrix_begin(elba_ctx *ctx, int nranks, const uint64_t *read_bounds, uint64_t *send_counts)
{
    return guarded(ctx, [&](Ctx &c) { stage_seed_matrix_begin(c, nranks, read_bounds, send_counts); });
}

int elba_set_stream(elba_ctx *ctx, void *hip_stream)
{
    return guarded(ctx, [&](Ctx &c) {
        if (c.stream) ELBA_HIP(hipStreamSynchronize(c.stream));
        if (c.own_stream && c.stream) (void)hipStreamDestroy(c.stream);
        c.stream = static_cast<hipStream_t>(hip_stream);
        c.own_stream = false;
    });
}

int elba_seed_matrix_send(elba_ctx *ctx, int nranks, const uint64_t *read_bounds, void *d_send, int64_t slot_records)
{
    return guarded(ctx, [&](Ctx &c) { stage_seed_matrix_send(c, nranks, read_bounds, d_send, slot_records); });
}

int elba_seed_matrix_recv(elba_ctx *ctx, void *d_recv, int64_t slot_records, elba_overlap_stats *stats, int64_t *slot_records_needed)
{
    bool done = false;
    const int rc = guarded(ctx, [&](Ctx &c) {
        done = stage_seed_matrix_recv(c, d_recv, slot_records, slot_records_needed);
        if (done && stats) *stats = c.ostats;
    });
    return rc != ELBA_OK ? rc : (done ? ELBA_OK : ELBA_ERR_RETRY);
}

int elba_seed_matrix_fill(elba_ctx *ctx, void *d_send, const uint64_t *offsets)
{
    return guarded(ctx, [&](Ctx &c) {
        ELBA_REQUIRE(offsets, ELBA_ERR_INVALID_ARG, "seed_matrix_fill: null offsets");
        stage_seed_matrix_fill(c, d_send, offsets);
    });
}

int elba_seed_matrix_end(elba_ctx *ctx, const void *d_recv, int64_t nrecords, elba_overlap_stats *stats)
{
    return guarded(ctx, [&](Ctx &c) {
        stage_seed_matrix_end(c, d_recv, nrecords);
        if (stats) *stats = c.ostats;
    });
}

int elba_align_seeds(elba_ctx *ctx, int mat, int mis, int gap, int dropoff, elba_align_stats *stats)
{
    return guarded(ctx, [&](Ctx &c) {
        stage_align_seeds(c, mat, mis, gap, dropoff);
        if (stats) *stats = c.astats;
    });
}

int elba_dist_set_all_reads(elba_ctx *ctx, const void *d_packed, int64_t packed_bytes, const void *d_byte_off, const void *d_len, int64_t nreads_total)
{
    return guarded(ctx, [&](Ctx &c) { stage_dist_set_all_reads(c, d_packed, packed_bytes, d_byte_off, d_len, nreads_total); });
}

int elba_export_overlaps(elba_ctx *ctx, elba_overlaps_t *out)
{
    return guarded(ctx, [&](Ctx &c) {
        ELBA_REQUIRE(out, ELBA_ERR_INVALID_ARG, "export_overlaps: null output");
        memset(out, 0, sizeof(*out));
        ELBA_REQUIRE(has(c.v, P_ALN), ELBA_ERR_STATE, "export_overlaps: no alignments (call elba_align_seeds)");
        const int64_t n = c.naln;
        out->n = n;
        out->rows = host_block<int64_t>((size_t)n); out->cols = host_block<int64_t>((size_t)n); out->vals = host_block<elba_overlap_t>((size_t)n);
        copy_out(c, out->rows, c.aln_rows.p, (size_t)n); copy_out(c, out->cols, c.aln_cols.p, (size_t)n); copy_out(c, out->vals, c.aln_out.p, (size_t)n);
        ELBA_HIP(hipStreamSynchronize(c.stream));
        for (int64_t a = 0; a < n; ++a) { out->rows[a] += c.first_global_id_rows(); out->cols[a] += c.first_global_id_rows(); }
    });
}

void elba_free_overlaps(elba_overlaps_t *o)
{
    if (!o) return;
    free(o->rows); free(o->cols); free(o->vals);
    memset(o, 0, sizeof(*o));
}

int elba_set_overlaps(elba_ctx *ctx, int64_t nreads, const int64_t *rows, const int64_t *cols, const elba_overlap_t *vals, int64_t n)
{
    return guarded(ctx, [&](Ctx &c) { stage_set_overlaps(c, nreads, rows, cols, vals, n); });
}

int elba_set_overlaps_device(elba_ctx *ctx, int64_t nreads, const void *d_rows, const void *d_cols, const void *d_vals, int64_t n)
{
    return guarded(ctx, [&](Ctx &c) { stage_set_overlaps_device(c, nreads, d_rows, d_cols, d_vals, n); });
}

int elba_set_outside_counts(elba_ctx *ctx, int64_t nreads, const uint32_t *aligned, const uint32_t *passed)
{
    return guarded(ctx, [&](Ctx &c) { stage_set_outside_counts(c, nreads, aligned, passed, false); });
}

int elba_set_outside_counts_device(elba_ctx *ctx, int64_t nreads, const void *d_aligned, const void *d_passed)
{
    return guarded(ctx, [&](Ctx &c) { stage_set_outside_counts(c, nreads, d_aligned, d_passed, true); });
}

int elba_transitive_reduction(elba_ctx *ctx, double bad_read_cutoff, int fuzz, elba_string_stats *stats)
{
    return guarded(ctx, [&](Ctx &c) {
        stage_transitive_reduction(c, bad_read_cutoff, fuzz);
        if (stats) *stats = c.sstats;
    });
}

int elba_export_string_graph(elba_ctx *ctx, elba_overlaps_t *out)
{
    return guarded(ctx, [&](Ctx &c) {
        ELBA_REQUIRE(out, ELBA_ERR_INVALID_ARG, "export_string_graph: null output");
        memset(out, 0, sizeof(*out));
        ELBA_REQUIRE(has(c.v, P_S), ELBA_ERR_STATE, "export_string_graph: no string graph (call elba_transitive_reduction)");
        const int64_t n = c.tr_nnz;
        out->n = n;
        out->rows = host_block<int64_t>((size_t)n); out->cols = host_block<int64_t>((size_t)n); out->vals = host_block<elba_overlap_t>((size_t)n);
        copy_out(c, out->rows, c.tr_out_rows.p, (size_t)n); copy_out(c, out->cols, c.tr_out_cols.p, (size_t)n); copy_out(c, out->vals, c.tr_out_vals.p, (size_t)n);
        ELBA_HIP(hipStreamSynchronize(c.stream));
        for (int64_t a = 0; a < n; ++a) { out->rows[a] += c.tr_id_base; out->cols[a] += c.tr_id_base; }
    });
}

int elba_export_read_flags(elba_ctx *ctx, uint8_t *flags, int64_t nreads)
{
    return guarded(ctx, [&](Ctx &c) {
        ELBA_REQUIRE(has(c.v, P_S), ELBA_ERR_STATE, "export_read_flags: no string graph (call elba_transitive_reduction)");
        ELBA_REQUIRE(nreads == c.tr_M && (flags || nreads == 0), ELBA_ERR_INVALID_ARG, "export_read_flags: need one byte per read of the graph");
        if (nreads) ELBA_HIP(hipMemcpyAsync(flags, c.tr_flags.p, (size_t)nreads, hipMemcpyDeviceToHost, c.stream));
        ELBA_HIP(hipStreamSynchronize(c.stream));
    });
}

int elba_clip_tips(elba_ctx *ctx, const elba_tip_cfg *cfg, elba_tip_stats *stats)
{
    return guarded(ctx, [&](Ctx &c) {
        stage_clip_tips(c, cfg);
        if (stats) *stats = c.tp.stats;
    });
}

int elba_pop_bubbles(elba_ctx *ctx, const elba_bubble_cfg *cfg, elba_bubble_stats *stats)
{
    return guarded(ctx, [&](Ctx &c) {
        stage_pop_bubbles(c, cfg);
        if (stats) *stats = c.bb.stats;
    });
}

int elba_cut_weak_overlaps(elba_ctx *ctx, const elba_weak_cfg *cfg, elba_weak_stats *stats)
{
    return guarded(ctx, [&](Ctx &c) {
        stage_cut_weak_overlaps(c, cfg);
        if (stats) *stats = c.wk.stats;
    });
}

int elba_cut_bridges(elba_ctx *ctx, const elba_bridge_cfg *cfg, elba_bridge_stats *stats)
{
    return guarded(ctx, [&](Ctx &c) {
        stage_cut_bridges(c, cfg);
        if (stats) *stats = c.br.stats;
    });
}

int elba_resolve_stars(elba_ctx *ctx, const elba_star_cfg *cfg, elba_star_stats *stats)
{
    return guarded(ctx, [&](Ctx &c) {
        stage_resolve_stars(c, cfg);
        if (stats) *stats = c.sr.stats;
    });
}

int elba_generate_contigs(elba_ctx *ctx, elba_contig_stats *stats)
{
    return guarded(ctx, [&](Ctx &c) {
        stage_generate_contigs(c, 0);
        if (stats) *stats = c.cg.stats;
    });
}

int elba_generate_contigs_ex(elba_ctx *ctx, const elba_contig_cfg *cfg, elba_contig_stats *stats)
{
    return guarded(ctx, [&](Ctx &c) {
        stage_generate_contigs_ex(c, cfg);
        if (stats) *stats = c.cg.stats;
    });
}

int elba_export_contigs(elba_ctx *ctx, elba_contigs_t *out)
{
    return guarded(ctx, [&](Ctx &c) {
        ELBA_REQUIRE(out, ELBA_ERR_INVALID_ARG, "export_contigs: null output");
        memset(out, 0, sizeof(*out));
        ELBA_REQUIRE(has(c.v, P_S, P_CONTIGS), ELBA_ERR_STATE, "export_contigs: no contigs of the current string graph (call elba_generate_contigs)");
        const int64_t n = c.cg.n, E = c.cg.E, b = c.cg.bases;
        elba_contigs_t o{};
        o.n = n;
        o.seq_off = host_block<int64_t>((size_t)n + 1); o.seq = host_block<char>((size_t)b); o.chain_off = host_block<int64_t>((size_t)n + 1);
        o.chain_read = host_block<int64_t>((size_t)E); o.chain_prefix = host_block<int32_t>((size_t)E); o.chain_strand = host_block<uint8_t>((size_t)E);
        *out = o;                                                   // (allocated before any copy: elba_free_contigs releases them if a copy fails)
        copy_out(c, o.seq_off, c.cg.soff.p, (size_t)n + 1); copy_out(c, o.chain_off, c.cg.coff.p, (size_t)n + 1); copy_out(c, o.seq, c.cg.seq.p, (size_t)b);
        copy_out(c, o.chain_read, c.cg.eread.p, (size_t)E); copy_out(c, o.chain_prefix, c.cg.epre.p, (size_t)E); copy_out(c, o.chain_strand, c.cg.estr.p, (size_t)E);
        ELBA_HIP(hipStreamSynchronize(c.stream));
    });
}

void elba_free_contigs(elba_contigs_t *c)
{
    if (!c) return;
    free(c->seq_off); free(c->seq); free(c->chain_off); free(c->chain_read); free(c->chain_prefix); free(c->chain_strand);
    memset(c, 0, sizeof(*c));
}

int elba_export_read_contigs(elba_ctx *ctx, int64_t *contig_of_read, int64_t nreads)
{
    return guarded(ctx, [&](Ctx &c) {
        ELBA_REQUIRE(has(c.v, P_S, P_CONTIGS), ELBA_ERR_STATE, "export_read_contigs: no contigs of the current string graph (call elba_generate_contigs)");
        ELBA_REQUIRE(nreads == c.tr_M && (contig_of_read || nreads == 0), ELBA_ERR_INVALID_ARG, "export_read_contigs: need one entry per read of the graph");
        const std::vector<int32_t> h = download<int32_t>(c, c.cg.cid.p, (size_t)nreads);
        for (int64_t v = 0; v < nreads; ++v) contig_of_read[v] = h[(size_t)v];
    });
}

int elba_export_assembly_links(elba_ctx *ctx, elba_links_t *out, elba_graph_stats *stats)
{
    return guarded(ctx, [&](Ctx &c) {
        ELBA_REQUIRE(out, ELBA_ERR_INVALID_ARG, "export_assembly_links: null output");
        memset(out, 0, sizeof(*out));
        stage_export_assembly_links(c, out);
        if (stats) *stats = c.gl.stats;
    });
}

void elba_free_links(elba_links_t *l)
{
    if (!l) return;
    free(l->links);
    memset(l, 0, sizeof(*l));
}

int elba_place_reads(elba_ctx *ctx, const elba_place_cfg *cfg, elba_placements_t *out, elba_place_stats *stats)
{
    if (out) memset(out, 0, sizeof(*out));                        // (before anything can fail: what is freed below is this call's)
    const int rc = guarded(ctx, [&](Ctx &c) {
        ELBA_REQUIRE(out, ELBA_ERR_INVALID_ARG, "place_reads: null output");
        stage_place_reads(c, cfg, out);
        if (stats) *stats = c.pl.stats;
    });
    if (rc != ELBA_OK && ctx && out) elba_free_placements(out);      // (a copy that failed behind the allocations)
    return rc;
}

int elba_polish_contigs(elba_ctx *ctx, const elba_polish_cfg *cfg, elba_polished_t *out, elba_polish_stats *stats)
{
    if (out) memset(out, 0, sizeof(*out));                        // (before anything can fail: what is freed below is this call's)
    const int rc = guarded(ctx, [&](Ctx &c) {
        ELBA_REQUIRE(out, ELBA_ERR_INVALID_ARG, "polish_contigs: null output");
        stage_polish_contigs(c, cfg, out);
        if (stats) *stats = c.po.stats;
    });
    if (rc != ELBA_OK && ctx && out) elba_free_polished(out);      // (a copy that failed behind the allocations)
    return rc;
}

int elba_graph_components(elba_ctx *ctx, const elba_cc_cfg *cfg, elba_components_t *out, elba_cc_stats *stats)
{
    if (out) memset(out, 0, sizeof(*out));                        // (before anything can fail: what is freed below is this call's)
    const int rc = guarded(ctx, [&](Ctx &c) {
        ELBA_REQUIRE(out, ELBA_ERR_INVALID_ARG, "graph_components: null output");
        stage_graph_components(c, cfg, out);
        if (stats) *stats = c.cc.stats;
    });
    if (rc != ELBA_OK && ctx && out) elba_free_components(out);      // (a copy that failed behind the allocations)
    return rc;
}

void elba_free_components(elba_components_t *p)
{
    if (!p) return;
    free(p->comp_of_read); free(p->first_read); free(p->reads); free(p->bases); free(p->edges); free(p->branches); free(p->ends);
    memset(p, 0, sizeof(*p));
}

int elba_partition_components(elba_ctx *ctx, const elba_part_cfg *cfg, int32_t *part_of_read, int64_t nreads, int64_t *part_weight)
{
    return guarded(ctx, [&](Ctx &c) { stage_partition_components(c, cfg, part_of_read, nreads, part_weight); });
}

int elba_induce_part(elba_ctx *ctx, const elba_induce_cfg *cfg, const int32_t *part_of_read, int64_t nreads, elba_induced_t *out, elba_induce_stats *stats)
{
    if (out) memset(out, 0, sizeof(*out));                        // (before anything can fail: what is freed below is this call's)
    const int rc = guarded(ctx, [&](Ctx &c) {
        stage_induce_part(c, cfg, part_of_read, nreads, out);
        if (stats) *stats = c.in.stats;
    });
    if (rc != ELBA_OK && ctx && out) elba_free_induced(out);      // (a copy that failed behind the allocations)
    return rc;
}

void elba_free_induced(elba_induced_t *o)
{
    if (!o) return;
    free(o->old_of_new); free(o->packed); free(o->byte_off); free(o->len); free(o->rows); free(o->cols); free(o->vals); free(o->outside_aligned); free(o->outside_passed);
    memset(o, 0, sizeof(*o));
}

void elba_free_polished(elba_polished_t *p)
{
    if (!p) return;
    free(p->seq_off); free(p->seq); free(p->voters); free(p->substituted); free(p->deleted); free(p->inserted); free(p->col_off); free(p->col); free(p->gap); free(p->reads);
    memset(p, 0, sizeof(*p));
}

void elba_free_placements(elba_placements_t *p)
{
    if (!p) return;
    free(p->reads); free(p->seg_off); free(p->seg_start); free(p->seg_depth); free(p->credited_reads); free(p->credited_bases);
    memset(p, 0, sizeof(*p));
}

int elba_export_contig_kinds(elba_ctx *ctx, uint8_t *kind, int64_t ncontigs)
{
    return guarded(ctx, [&](Ctx &c) {
        ELBA_REQUIRE(has(c.v, P_S, P_CONTIGS), ELBA_ERR_STATE, "export_contig_kinds: no contigs of the current string graph (call elba_generate_contigs)");
        ELBA_REQUIRE(ncontigs == c.cg.n && (kind || ncontigs == 0), ELBA_ERR_INVALID_ARG, "export_contig_kinds: need one byte per contig");
        if (ncontigs) ELBA_HIP(hipMemcpyAsync(kind, c.cg.kind.p, (size_t)ncontigs, hipMemcpyDeviceToHost, c.stream));
        ELBA_HIP(hipStreamSynchronize(c.stream));
    });
}

int elba_read_pileup(elba_ctx *ctx, const elba_pileup_cfg *cfg, elba_pileup_stats *stats)
{
    return guarded(ctx, [&](Ctx &c) {
        stage_read_pileup(c, cfg);
        if (stats) *stats = c.pu.stats;
    });
}

int elba_export_pileup(elba_ctx *ctx, elba_pileup_t *out)
{
    return guarded(ctx, [&](Ctx &c) {
        ELBA_REQUIRE(out, ELBA_ERR_INVALID_ARG, "export_pileup: null output");
        memset(out, 0, sizeof(*out));
        ELBA_REQUIRE(has(c.v, P_PILEUP), ELBA_ERR_STATE, "export_pileup: no pileup of the current overlaps (call elba_read_pileup)");
        const int64_t n = c.pu.M, S = c.pu.nseg;
        elba_pileup_t o{};
        o.n = n; o.nseg = S;
        o.seg_off = host_block<int64_t>((size_t)n + 1); o.seg_start = host_block<int32_t>((size_t)S); o.seg_depth = host_block<int32_t>((size_t)S);
        o.trim_beg = host_block<int32_t>((size_t)n); o.trim_end = host_block<int32_t>((size_t)n); o.flags = host_block<uint8_t>((size_t)n);
        *out = o;                                                   // (allocated before any copy: elba_free_pileup releases them if a copy fails)
        copy_out(c, o.seg_off, c.pu.depth.seg_off.p, (size_t)n + 1); copy_out(c, o.seg_start, c.pu.depth.seg_start.p, (size_t)S); copy_out(c, o.seg_depth, c.pu.depth.seg_depth.p, (size_t)S);
        std::vector<int32_t> trim((size_t)(2 * n));
        copy_out(c, trim.data(), c.pu.trim.p, (size_t)(2 * n)); copy_out(c, o.flags, c.pu.flags.p, (size_t)n);
        ELBA_HIP(hipStreamSynchronize(c.stream));
        for (int64_t v = 0; v < n; ++v) { o.trim_beg[v] = trim[(size_t)(2 * v)]; o.trim_end[v] = trim[(size_t)(2 * v + 1)]; }
    });
}

void elba_free_pileup(elba_pileup_t *p)
{
    if (!p) return;
    free(p->seg_off); free(p->seg_start); free(p->seg_depth); free(p->trim_beg); free(p->trim_end); free(p->flags);
    memset(p, 0, sizeof(*p));
}

int elba_prune_reads(elba_ctx *ctx, int mask, int64_t *kept)
{
    return guarded(ctx, [&](Ctx &c) { stage_prune_reads(c, mask, kept); });
}

int elba_trim_reads(elba_ctx *ctx, const elba_trim_cfg *cfg, elba_trim_stats *stats)
{
    return guarded(ctx, [&](Ctx &c) {
        stage_trim_reads(c, cfg);
        if (stats) *stats = c.tm.stats;
    });
}

int elba_export_trim_map(elba_ctx *ctx, elba_trim_map_t *out)
{
    return guarded(ctx, [&](Ctx &c) {
        ELBA_REQUIRE(out, ELBA_ERR_INVALID_ARG, "export_trim_map: null output");
        memset(out, 0, sizeof(*out));
        ELBA_REQUIRE(has(c.v, P_TRIM), ELBA_ERR_STATE, "export_trim_map: no trimmed reads (call elba_trim_reads)");
        const int64_t n = c.tm.n;
        elba_trim_map_t o{};
        o.n = n;
        o.src_read = host_block<int64_t>((size_t)n); o.src_beg = host_block<int32_t>((size_t)n); o.src_end = host_block<int32_t>((size_t)n);
        *out = o;                                                   // (allocated before any copy: elba_free_trim_map releases them if a copy fails)
        copy_out(c, o.src_read, c.tm.src.p, (size_t)n); copy_out(c, o.src_beg, c.tm.beg.p, (size_t)n); copy_out(c, o.src_end, c.tm.end.p, (size_t)n);
        ELBA_HIP(hipStreamSynchronize(c.stream));
    });
}

void elba_free_trim_map(elba_trim_map_t *m)
{
    if (!m) return;
    free(m->src_read); free(m->src_beg); free(m->src_end);
    memset(m, 0, sizeof(*m));
}

int elba_get_trimmed_reads_device(elba_ctx *ctx, const void **d_packed, int64_t *packed_bytes, const void **d_byte_off, const void **d_len, int64_t *n)
{
    return guarded(ctx, [&](Ctx &c) {
        ELBA_REQUIRE(d_packed && packed_bytes && d_byte_off && d_len && n, ELBA_ERR_INVALID_ARG, "get_trimmed_reads_device: null output");
        ELBA_REQUIRE(has(c.v, P_TRIM), ELBA_ERR_STATE, "get_trimmed_reads_device: no trimmed reads (call elba_trim_reads)");
        *d_packed = c.tm.packed.p; *packed_bytes = c.tm.packed_bytes; *d_byte_off = c.tm.off.p; *d_len = c.tm.len.p; *n = c.tm.n;
    });
}

int elba_adopt_trimmed_reads(elba_ctx *ctx)
{
    return guarded(ctx, [&](Ctx &c) { stage_adopt_trimmed_reads(c); });
}

int elba_export_csr(elba_ctx *ctx, int64_t row_lo, int64_t row_hi, elba_csr_t *out)
{
    return guarded(ctx, [&](Ctx &c) {
        ELBA_REQUIRE(out, ELBA_ERR_INVALID_ARG, "export_csr: null output");
        memset(out, 0, sizeof(*out));
        ELBA_REQUIRE(has(c.v, P_B), ELBA_ERR_STATE, "export_csr: no seed matrix");
        ELBA_REQUIRE(row_lo >= 0 && row_lo <= row_hi && row_hi <= c.M, ELBA_ERR_INVALID_ARG, "export_csr: bad row range");
        auto rp = download<int64_t>(c, c.b_rowptr.as<int64_t>() + row_lo, (size_t)(row_hi - row_lo + 1));
        const int64_t e0 = rp.front(), e1 = rp.back(), n = e1 - e0;
        auto col = download<uint32_t>(c, c.b_col.as<uint32_t>() + e0, (size_t)n);
        out->nrows = row_hi - row_lo; out->ncols = c.M; out->nnz = n;
        out->rowptr = host_block<int64_t>((size_t)(row_hi - row_lo + 1));
        out->col = host_block<int64_t>((size_t)n);
        out->val = host_block<elba_seed_t>((size_t)n);
        for (size_t i = 0; i < rp.size(); ++i) out->rowptr[i] = rp[i] - e0;
        for (int64_t i = 0; i < n; ++i) out->col[i] = col[(size_t)i];
        copy_out(c, out->val, c.b_val.as<elba_seed_t>() + e0, (size_t)n);
        ELBA_HIP(hipStreamSynchronize(c.stream));
    });
}

void elba_free_csr(elba_csr_t *c)
{
    if (!c) return;
    free(c->rowptr); free(c->col); free(c->val);
    memset(c, 0, sizeof(*c));
}

int elba_export_dcsc(elba_ctx *ctx, int64_t row_lo, int64_t row_hi, int64_t col_lo, int64_t col_hi, elba_dcsc_t *out)
{
    return guarded(ctx, [&](Ctx &c) {
        ELBA_REQUIRE(out, ELBA_ERR_INVALID_ARG, "export_dcsc: null output");
        memset(out, 0, sizeof(*out));
        ELBA_REQUIRE(has(c.v, P_B), ELBA_ERR_STATE, "export_dcsc: no seed matrix");
        ELBA_REQUIRE(row_lo >= 0 && row_lo <= row_hi && row_hi <= c.M && col_lo >= 0 && col_lo <= col_hi && col_hi <= c.M, ELBA_ERR_INVALID_ARG, "export_dcsc: bad block");
        // rows [row_lo,row_hi) of the device CSR -> host; column-major regrouping is index bookkeeping on the exported copy
        auto rp = download<int64_t>(c, c.b_rowptr.as<int64_t>() + row_lo, (size_t)(row_hi - row_lo + 1));
        const int64_t e0 = rp.front(), n = rp.back() - e0;
        auto col = download<uint32_t>(c, c.b_col.as<uint32_t>() + e0, (size_t)n);
        auto val = download<elba_seed_t>(c, c.b_val.as<elba_seed_t>() + e0, (size_t)n);
        const int64_t ncols = col_hi - col_lo;
        std::vector<int64_t> cnt((size_t)ncols + 1, 0);
        int64_t total = 0;
        for (int64_t e = 0; e < n; ++e) { int64_t j = col[(size_t)e]; if (j >= col_lo && j < col_hi) { cnt[(size_t)(j - col_lo)]++; ++total; } }
        int64_t nzc = 0;
        for (int64_t j = 0; j < ncols; ++j) if (cnt[(size_t)j]) ++nzc;
        out->nrows = row_hi - row_lo; out->ncols = ncols; out->nnz = total; out->nzc = nzc;
        out->jc = host_block<int64_t>((size_t)nzc);
        out->cp = host_block<int64_t>((size_t)nzc + 1);
        out->ir = host_block<int64_t>((size_t)total);
        out->numx = host_block<elba_seed_t>((size_t)total);
        std::vector<int64_t> start((size_t)ncols + 1, 0);
        int64_t run = 0, ci = 0;
        for (int64_t j = 0; j < ncols; ++j) {
            start[(size_t)j] = run;
            if (cnt[(size_t)j]) { out->jc[ci] = j; out->cp[ci] = run; ++ci; }
            run += cnt[(size_t)j];
        }
        out->cp[nzc] = run;
        for (int64_t r = 0; r < row_hi - row_lo; ++r)
            for (int64_t e = rp[(size_t)r] - e0; e < rp[(size_t)r + 1] - e0; ++e) {
                int64_t j = col[(size_t)e];
                if (j >= col_lo && j < col_hi) { int64_t d = start[(size_t)(j - col_lo)]++; out->ir[d] = r; out->numx[d] = val[(size_t)e]; }
            }
    });
}

void elba_free_dcsc(elba_dcsc_t *d)
{
    if (!d) return;
    free(d->jc); free(d->cp); free(d->ir); free(d->numx);
    memset(d, 0, sizeof(*d));
}

int elba_export_kmer_matrix(elba_ctx *ctx, elba_kmer_matrix_t *out)
{
    return guarded(ctx, [&](Ctx &c) {
        ELBA_REQUIRE(out, ELBA_ERR_INVALID_ARG, "export_kmer_matrix: null output");
        memset(out, 0, sizeof(*out));
        ELBA_REQUIRE(has(c.v, P_A), ELBA_ERR_STATE, "export_kmer_matrix: no k-mer matrix");
        const size_t M = (size_t)c.M, N = (size_t)c.N, Z = (size_t)c.Z;
        auto rp = download<uint32_t>(c, c.a_rowptr.p, M + 1);
        auto cp = download<uint32_t>(c, c.a_colptr.p, N + 1);
        auto csr = download<uint64_t>(c, c.a_csr.p, Z);
        auto csc = download<uint64_t>(c, c.a_csc.p, Z);
        out->nrows = c.M; out->ncols = c.N; out->nnz = c.Z;
        out->colptr = host_block<int64_t>(N + 1); out->rowptr = host_block<int64_t>(M + 1);
        out->csc_row = host_block<int64_t>(Z); out->csc_val = host_block<uint32_t>(Z);
        out->csr_col = host_block<int64_t>(Z); out->csr_val = host_block<uint32_t>(Z);
        for (size_t i = 0; i <= N; ++i) out->colptr[i] = cp[i];
        for (size_t i = 0; i <= M; ++i) out->rowptr[i] = rp[i];
        for (size_t z = 0; z < Z; ++z) {
            out->csc_row[z] = (int64_t)(csc[z] >> 32) + c.first_global_id_rows(); out->csc_val[z] = (uint32_t)csc[z];
            out->csr_col[z] = (int64_t)(csr[z] >> 32); out->csr_val[z] = (uint32_t)csr[z] & csr_pos_mask(c.csr_suffix, c.csr_hints);      // (above the position: SpGEMM hints, or column length and place of a dense matrix)
        }
        if (c.csr_inline) {
            // rows with inline partners (Ctx::csr_inline) do not name the k-mer of such an entry: the rows are rebuilt from the columns — walked in
            // k-mer order, every column's entries in (read, pos) order, a row fills up in (k-mer id, pos) order
            std::vector<size_t> fill(rp.begin(), rp.end() - 1);
            for (size_t k = 0; k < N; ++k)
                for (size_t z = cp[k]; z < cp[k + 1]; ++z) { const size_t at = fill[(size_t)(csc[z] >> 32)]++; out->csr_col[at] = (int64_t)k; out->csr_val[at] = (uint32_t)csc[z]; }
        }
        if (c.A_has_kmers) {
            out->kmers = host_block<uint64_t>(N);
            copy_out(c, out->kmers, c.rel_kmers.p, N);
            if (c.cfg.k > 32) {
                out->kmers_lo = host_block<uint64_t>(N);
                copy_out(c, out->kmers_lo, c.rel_kmers_lo.p, N);
            }
            if (c.cfg.k > 64) {
                out->kmers_lo2 = host_block<uint64_t>(N);
                copy_out(c, out->kmers_lo2, c.rel_kmers_lo2.p, N);
            }
            ELBA_HIP(hipStreamSynchronize(c.stream));
        }
    });
}

void elba_free_kmer_matrix(elba_kmer_matrix_t *m)
{
    if (!m) return;
    free(m->kmers); free(m->kmers_lo); free(m->kmers_lo2); free(m->colptr); free(m->csc_row); free(m->csc_val); free(m->rowptr); free(m->csr_col); free(m->csr_val);
    memset(m, 0, sizeof(*m));
}

int elba_kmer_histogram(elba_ctx *ctx, int64_t *hist, int64_t len)
{
    return guarded(ctx, [&](Ctx &c) {
        ELBA_REQUIRE(hist && len > 0, ELBA_ERR_INVALID_ARG, "kmer_histogram: null output");
        ELBA_REQUIRE(has(c.v, P_A), ELBA_ERR_STATE, "kmer_histogram: no k-mer matrix");
        auto cp = download<uint32_t>(c, c.a_colptr.p, (size_t)c.N + 1);
        for (int64_t i = 0; i < len; ++i) hist[i] = 0;
        for (int64_t k = 0; k < c.N; ++k) { int64_t n = (int64_t)cp[(size_t)k + 1] - cp[(size_t)k]; if (n < len) hist[n]++; }
    });
}

static_assert((int)CSR_FORMAT_PLAIN == ELBA_CSR_PLAIN && (int)CSR_FORMAT_HINTS == ELBA_CSR_HINTS && (int)CSR_FORMAT_DENSE == ELBA_CSR_DENSE && (int)CSR_FORMAT_INLINE == ELBA_CSR_INLINE, "csr_plan.hpp numbers the formats as the ABI does");
int elba_get_device_view(elba_ctx *ctx, elba_device_view *v)
{
    return guarded(ctx, [&](Ctx &c) {
        ELBA_REQUIRE(v, ELBA_ERR_INVALID_ARG, "get_device_view: null output");
        memset(v, 0, sizeof(*v));
        v->stream = (void *)c.stream;
        if (has(c.v, P_A)) { v->M = c.M; v->N = c.N; v->Z = c.Z; v->a_rowptr = c.a_rowptr.p; v->a_csr = c.a_csr.p; v->a_colptr = c.a_colptr.p; v->a_csc = c.a_csc.p;
                        v->a_csr_format = csr_format(c.csr_inline, c.csr_suffix, c.csr_hints);
                        v->a_csr_pos_mask = csr_pos_mask(c.csr_suffix, c.csr_hints);
                        v->a_kmers = c.A_has_kmers ? c.rel_kmers.p : nullptr;
                        v->a_gather_slots = c.use_ell && c.ell_compact ? c.ell_nslots : 0;
                        v->a_slot_kid = c.use_ell && c.ell_compact ? c.ell_slot_kid.p : nullptr; }
        if (has(c.v, P_B)) { v->Y = c.Y; v->b_rowptr = c.b_rowptr.p; v->b_col = c.b_col.p; v->b_val = c.b_val.p; }
    });
}

int elba_set_option(elba_ctx *ctx, const char *name, int64_t value)
{
    return guarded(ctx, [&](Ctx &c) {
        ELBA_REQUIRE(name, ELBA_ERR_INVALID_ARG, "set_option: null name");
        struct { const char *n; bool *b; } flags[] = {
            {"overlap_cold_calls", &c.cold_calls}, {"no_symmetry", &c.opt.no_symmetry}, {"no_ell", &c.opt.no_ell}, {"no_pay", &c.opt.no_pay}, {"mir32", &c.opt.mir32},
            {"no_hints", &c.opt.no_hints}, {"no_sample", &c.opt.no_sample}, {"no_slab", &c.opt.no_slab}, {"no_ell_compact", &c.opt.no_ell_compact}, {"msd_no_rank", &c.opt.msd_no_rank}, {"msd_rank", &c.opt.msd_rank}, {"csr_pairs_late", &c.opt.csr_pairs_late}, {"no_suffix", &c.opt.no_suffix}, {"no_row_order", &c.opt.no_row_order}, {"no_inline", &c.opt.no_inline}, {"panel_inline", &c.opt.panel_inline}, {"kmer_pairs", &c.opt.kmer_pairs},
            {"kmer_unfused", &c.opt.kmer_unfused}, {"kmer_no_msd", &c.opt.kmer_no_msd}, {"kmer_msd", &c.opt.kmer_msd}, {"csr_pairs", &c.opt.csr_pairs}, {"emit_plain", &c.opt.emit_plain}, {"trace", &c.opt.trace}, {"measure_prep", &c.opt.measure_prep}};
        for (auto &f : flags) if (!strcmp(name, f.n)) { *f.b = value != 0; return; }
        // "ov_generic" (A/B of the numeric kernel on reads-built matrices): 0 the kernel the plan picks, 1 the general kernel, 2 the reads path with run-time geometry
        if (!strcmp(name, "ov_generic")) { ELBA_REQUIRE(value >= 0 && value <= 2, ELBA_ERR_INVALID_ARG, "set_option: ov_generic is 0, 1 or 2"); c.opt.ov_generic = value == 1; c.opt.ov_spec_rt_geom = value == 2; }
        else if (!strcmp(name, "kmer_drop")) { ELBA_REQUIRE(value >= 0 && value <= 3, ELBA_ERR_INVALID_ARG, "set_option: kmer_drop is 0..3"); c.opt.kmer_drop = (int)value; }
        else if (!strcmp(name, "dense_up")) { ELBA_REQUIRE(value >= 0 && value <= 3, ELBA_ERR_INVALID_ARG, "set_option: dense_up is 0..3"); c.opt.dense_up = (int)value; }
        else if (!strcmp(name, "dense_wgs")) { ELBA_REQUIRE(value >= 1 && value <= 16, ELBA_ERR_INVALID_ARG, "set_option: dense_wgs is 1..16"); c.opt.dense_wgs = (int)value; }
        else if (!strncmp(name, "tune", 4) && name[4] >= '1' && name[4] <= '7' && name[4] != '6' && name[5] == 0) c.opt.tune[name[4] - '0'] = value;      // ("tune0" and "tune6" are retired: unknown names)
        else if (!strcmp(name, "msd_small_cap")) c.opt.msd_small_cap = (int)value;
        else if (!strcmp(name, "kmer_batch_instances")) { ELBA_REQUIRE(value >= 0, ELBA_ERR_INVALID_ARG, "set_option: kmer_batch_instances is >= 0"); c.opt.kmer_batch_instances = value; }
        else if (!strcmp(name, "msd_wide_bits")) c.opt.msd_wide_bits = (int)value;
        else if (!strcmp(name, "ell_slot_cap")) c.opt.ell_slot_cap = (int)value;
        else if (!strcmp(name, "slab_pct")) { ELBA_REQUIRE(value >= 1 && value <= 1000, ELBA_ERR_INVALID_ARG, "set_option: slab_pct is 1..1000"); c.opt.slab_pct = (int)value; }
        else if (!strcmp(name, "slab_q16")) { ELBA_REQUIRE(value >= 0 && value < (1ll << 31), ELBA_ERR_INVALID_ARG, "set_option: slab_q16 is 0..2^31"); c.opt.slab_q16 = (int)value; }
        else if (!strcmp(name, "dk")) { ELBA_REQUIRE(value == -1 || value == 0 || value == 1 || value == 2 || value == 4, ELBA_ERR_INVALID_ARG, "set_option: dk is -1 (chosen per matrix), 0, 1, 2 or 4"); c.opt.dk = (int)value; }
        else if (!strcmp(name, "aln_tiers")) { ELBA_REQUIRE(value >= 0, ELBA_ERR_INVALID_ARG, "set_option: aln_tiers is a string of the digits 1, 2, 4, 8"); c.opt.aln_tiers = value; }
        else if (!strcmp(name, "aln_wide_hint")) c.opt.aln_wide_hint = (int)value;
        else if (!strcmp(name, "aln_long_hint")) c.opt.aln_long_hint = (int)value;
        else if (!strcmp(name, "polish_trace_bytes")) { ELBA_REQUIRE(value >= 0, ELBA_ERR_INVALID_ARG, "set_option: polish_trace_bytes is >= 0"); c.opt.polish_trace_bytes = value; }
        else throw Error{ELBA_ERR_INVALID_ARG, std::string("set_option: unknown option ") + name};
    });
}

int elba_release_workspace(elba_ctx *ctx)
{
    return guarded(ctx, [&](Ctx &c) {
        ELBA_REQUIRE(!c.dist_owner && c.ov_phase == 0, ELBA_ERR_STATE, "release_workspace: the context holds exchanged records or is inside a sharded multiplication");
        ELBA_HIP(hipStreamSynchronize(c.stream));
        c.ws_a.release(); c.ws_b.release(); c.ws_c.release(); c.ws_d.release(); c.ws_e.release(); c.ws_f.release(); c.ws_g.release(); c.ws_h.release(); c.ws_sort.release();
        c.csr_words.release(); c.kid_of_entry.release();
        // the late stages: what each keeps is its release_scratch()'s decision (common.hpp, the stage structs of Ctx)
        c.cg.release_scratch(); c.gl.release_scratch(); c.pu.release_scratch(); c.pl.release_scratch(); c.po.release_scratch(); c.cc.release_scratch(); c.in.release_scratch(); c.tm.release_scratch();
        c.sg.release();      // the cleaning calls' shared scratch and the spare buffer of S (S itself stays)
        c.tp.release_scratch(); c.bb.release_scratch(); c.wk.release_scratch(); c.br.release_scratch(); c.sr.release_scratch();
        if (has(c.v, P_COUNTS)) c.pre.consume();    // (the CSR sort keys / column ids of the entries are gone: create_kmer_matrix rebuilds them from the column pointers)
    });
}

int elba_get_stat(elba_ctx *ctx, const char *name, int64_t *value)
{
    return guarded(ctx, [&](Ctx &c) {
        ELBA_REQUIRE(name && value, ELBA_ERR_INVALID_ARG, "get_stat: null name or value");
        if (!strcmp(name, "overlap_mirror_placed")) *value = c.ov_mir_placed;
        else if (!strcmp(name, "overlap_slab_q16")) *value = (int64_t)c.ov_slab_q16_used;
        else if (!strcmp(name, "kmer_path")) *value = c.kmer_path;
        else if (!strcmp(name, "kmer_passes")) *value = c.kmer_passes;      // value-range passes the last elba_count_kmers took (1: the whole input at once)
        else if (!strcmp(name, "kmer_crowded_buckets")) *value = c.kmer_crowded;      // buckets the last elba_count_kmers gave up to a crowded path (wide: k31_count's crowded parents; k <= 17: k_msd_bucket's)
        else if (!strcmp(name, "kmer_crowded_small")) *value = c.kmer_crowded_small;      // wide crowded parents whose folded entry count lies in (0, small_cap]: what the main emit classes would take
        else if (!strcmp(name, "kmer_largest_pass")) *value = c.kmer_largest_pass;      // instances of the last elba_count_kmers' largest value-range pass (I when unbatched)
        else if (!strcmp(name, "kmer_peak_bytes")) *value = c.kmer_peak_bytes;      // device bytes the last elba_count_kmers' value-range passes of k > 31 held at their high point (0: not batched)
        else if (!strcmp(name, "kmer_buckets")) *value = c.kmer_buckets;      // buckets of the last elba_count_kmers' value partition, all passes (0: the sort)
        else if (!strcmp(name, "overlap_passes")) *value = c.ov_passes;      // passes the last create_seed_matrix took (1: no repeat; set also when the call failed)
        else if (!strcmp(name, "overlap_spec")) *value = c.ov_spec;      // 1: the last create_seed_matrix ran the reads-path instantiation of the numeric kernel (ov_plan.hpp: ov_spec_ok), 0: the general one
        else if (!strcmp(name, "overlap_spec_geom")) *value = c.ov_spec_geom;      // 1: ... and its compiled-geometry variant (table size, claim limit and column geometry are constants: ov_spec_geom_ok)
        else if (!strcmp(name, "overlap_forwarded")) *value = c.ov_forwarded;      // rows the last create_seed_matrix forwarded to a larger tier on a prediction, all passes
        // where the rows of the last create_seed_matrix went (its final pass) and on which shape of A it ran: read-only, for tests that place a row on a constant
        else if (!strncmp(name, "overlap_tier_limit_", 19) && name[19] >= '0' && name[19] < '0' + NUM_LDS_TIERS && !name[20]) *value = c.ov_tier_limit[name[19] - '0'];
        else if (!strncmp(name, "overlap_tier_queued_", 20) && name[20] >= '0' && name[20] < '0' + NUM_TIERS && !name[21]) *value = c.ov_tier_queued[name[20] - '0'];
        else if (!strncmp(name, "overlap_tier_done_", 18) && name[18] >= '0' && name[18] < '0' + NUM_TIERS && !name[19]) *value = c.ov_tier_done[name[18] - '0'];
        else if (!strcmp(name, "overlap_sort_rows_bucket")) *value = c.ov_sort_rows[0];
        else if (!strcmp(name, "overlap_sort_rows_huge")) *value = c.ov_sort_rows[1];
        else if (!strcmp(name, "overlap_family")) *value = c.ov_family;
        else if (!strcmp(name, "overlap_pay16")) *value = c.ov_pay16;
        else if (!strcmp(name, "overlap_rec16")) *value = c.ov_rec16_used;
        else if (!strcmp(name, "matrix_col_stride")) *value = has(c.v, P_A) && c.use_ell ? (int64_t)c.s_stride : 0;
        else if (!strcmp(name, "matrix_fbits")) *value = has(c.v, P_A) ? (int64_t)c.fbits : 0;
        else if (!strcmp(name, "matrix_pos16")) *value = has(c.v, P_A) && c.pos16 ? 1 : 0;
        else if (!strcmp(name, "matrix_hints")) *value = has(c.v, P_A) && c.csr_hints ? 1 : 0;
        else if (!strcmp(name, "matrix_inline")) *value = has(c.v, P_A) && c.csr_inline ? 1 : 0;
        else if (!strcmp(name, "matrix_suffix")) *value = has(c.v, P_A) && c.csr_suffix ? 1 : 0;
        else if (!strcmp(name, "matrix_csr_words")) *value = has(c.v, P_A) && c.csr_one_word ? 1 : 0;
        else if (!strcmp(name, "spgemm_prep_us")) *value = c.prep_us;     // (option "measure_prep"; -1: not measured — the option was off, or the path taken has no emit kernels of its own)
        else if (!strcmp(name, "emit_us")) *value = c.emit_us;
        else if (!strcmp(name, "triples_path")) *value = c.triples_path;
        else if (!strcmp(name, "text_tile_bytes")) *value = TEXT_TILE_BYTES;      // constants of elba_set_reads_text: the bytes of a tile of its two passes over the chunk,
        else if (!strcmp(name, "text_scan_span")) *value = scan_block_span();      // and the elements beyond which its scans recurse (tests size their inputs from them)
        else if (!strcmp(name, "padded_columns")) *value = has(c.v, P_A) && c.use_ell ? 1 : 0;
        else if (!strcmp(name, "gather_slots")) *value = has(c.v, P_A) && c.use_ell ? c.ell_nslots : 0;
        else if (!strcmp(name, "contig_count")) *value = has(c.v, P_S, P_CONTIGS) ? c.cg.stats.contigs : 0;          // the last elba_generate_contigs (0: none valid — the condition of the contig exports)
        else if (!strcmp(name, "contig_cycles")) *value = has(c.v, P_S, P_CONTIGS) ? c.cg.stats.cycles : 0;
        else if (!strcmp(name, "contig_circular")) *value = has(c.v, P_S, P_CONTIGS) ? c.cg.circular : 0;
        else if (!strcmp(name, "contig_singletons")) *value = has(c.v, P_S, P_CONTIGS) ? c.cg.singletons : 0;
        else if (!strcmp(name, "contig_reads")) *value = has(c.v, P_S, P_CONTIGS) ? c.cg.stats.contig_reads : 0;
        else if (!strcmp(name, "contig_bases")) *value = has(c.v, P_S, P_CONTIGS) ? c.cg.stats.bases : 0;
        else if (!strcmp(name, "contig_branches")) *value = has(c.v, P_S, P_CONTIGS) ? c.cg.stats.branches : 0;
        // the last elba_export_assembly_links / elba_place_reads / elba_polish_contigs on the contigs that are valid now
        else if (!strncmp(name, "graph_", 6)) {
            using S = elba_graph_stats;
            static const StatName<S> table[] = {{"segments", &S::segments}, {"candidates", &S::candidates}, {"links", &S::links}, {"closures", &S::closures},
                                                {"twisted", &S::twisted}, {"unplaced", &S::unplaced}, {"clamped", &S::clamped}, {"asymmetric", &S::asymmetric}};
            *value = stage_stat(table, c.gl.stats, has(c.v, P_S, P_CONTIGS) && c.gl.for_cg == c.cg.serial, name + 6, name);
        }
        else if (!strncmp(name, "place_", 6)) {
            using S = elba_place_stats;
            static const StatName<S> table[] = {{"chain", &S::chain}, {"anchored", &S::anchored}, {"unanchored", &S::unanchored}, {"skipped", &S::skipped}, {"candidates", &S::candidates},
                                                {"clipped", &S::clipped}, {"outside", &S::outside}, {"wrapped", &S::wrapped}, {"segments", &S::segments}, {"max_depth", &S::max_depth}};
            *value = stage_stat(table, c.pl.stats, has(c.v, P_S, P_CONTIGS) && c.pl.for_cg == c.cg.serial && c.pl.for_cg != 0, name + 6, name);
        }
        else if (!strncmp(name, "polish_", 7)) {
            using S = elba_polish_stats;
            static const StatName<S> table[] = {{"voted", &S::voted}, {"rejected", &S::rejected}, {"outside", &S::outside}, {"low_depth_columns", &S::low_depth_columns},
                                                {"bases_before", &S::bases_before}, {"bases_after", &S::bases_after}, {"sum_dist", &S::sum_dist}, {"cells", &S::cells}, {"batches", &S::batches}};
            *value = stage_stat(table, c.po.stats, has(c.v, P_S, P_CONTIGS) && c.po.for_cg == c.cg.serial && c.po.for_cg != 0, name + 7, name);
        }
        // the last labelling (elba_graph_components / elba_partition_components), while the graph it labelled is valid
        else if (!strncmp(name, "cc_", 3)) {
            using S = elba_cc_stats;
            const bool valid = c.cc.graph == ELBA_CC_STRING ? has(c.v, P_S) : c.cc.graph == ELBA_CC_OVERLAPS && (has(c.v, P_EDGES) || has(c.v, P_ALN));
            if (!strcmp(name, "cc_passes")) *value = valid ? c.cc.stats.passes : 0;
            else {
                static const StatName<S> table[] = {{"components", &S::components}, {"used_components", &S::used_components}, {"largest_reads", &S::largest_reads}};
                *value = stage_stat(table, c.cc.stats, valid, name + 3, name);
            }
        }
        else if (!strcmp(name, "induce_reads")) *value = c.in.stats.reads;      // the last elba_induce_part that succeeded
        else if (!strcmp(name, "induce_pairs")) *value = c.in.stats.pairs;
        else if (!strcmp(name, "induce_split_pairs")) *value = c.in.stats.split_pairs;
        else if (!strcmp(name, "contig_rank_us")) *value = has(c.v, P_S, P_CONTIGS) ? (int64_t)(c.cg.stats.ms_rank * 1000.0f) : -1;
        else if (!strcmp(name, "resident_bytes_A")) {
            int64_t b = 0;
            if (has(c.v, P_A)) {
                b = (int64_t)(c.M + 1) * 4 + (int64_t)(c.N + 1) * 4 + 16 * c.Z;
                if (c.use_ell) b += 8 * c.ell_nslots * (int64_t)c.s_stride + (c.ell_compact ? 4 * c.ell_nslots : 0);
                if (c.csr_suffix) b += (4ll * c.N) << c.j_shift;
            }
            *value = b;
        }
        else throw Error{ELBA_ERR_INVALID_ARG, std::string("get_stat: unknown counter ") + name};
    });
}

int elba_kmer_hash_owner(elba_ctx *ctx, const uint64_t *kmers, int64_t n, int nprocs, uint64_t *hash, int32_t *owner)
{
    return guarded(ctx, [&](Ctx &c) { stage_ref_hash_owner(c, kmers, n, nprocs, hash, owner); });
}

int elba_dist_value_histogram(elba_ctx *ctx, uint64_t *hist, int64_t nbins)
{
    return guarded(ctx, [&](Ctx &c) { stage_dist_value_histogram(c, hist, nbins); });
}

int elba_dist_set_owner_ranges(elba_ctx *ctx, int nranks, const uint32_t *upper_bins)
{
    return guarded(ctx, [&](Ctx &c) { stage_dist_set_owner_ranges(c, nranks, upper_bins); });
}

int elba_dist_set_kmer_id_base(elba_ctx *ctx, int64_t base, int64_t nall)
{
    return guarded(ctx, [&](Ctx &c) { stage_dist_set_kmer_id_base(c, base, nall); });
}

int elba_dist_count_owners(elba_ctx *ctx, int nranks, uint64_t *counts)
{
    return guarded(ctx, [&](Ctx &c) {
        ELBA_REQUIRE(counts, ELBA_ERR_INVALID_ARG, "dist_count_owners: null output");
        stage_dist_count_owners(c, nranks, counts);
    });
}

int elba_dist_fill_send(elba_ctx *ctx, int nranks, void *d_send, const uint64_t *offsets)
{
    return guarded(ctx, [&](Ctx &c) {
        ELBA_REQUIRE(offsets && (d_send || c.I == 0), ELBA_ERR_INVALID_ARG, "dist_fill_send: null argument");
        stage_dist_fill_send(c, nranks, d_send, offsets);
    });
}

int elba_dist_packed_format(elba_ctx *ctx, int nranks, const int64_t *read_bounds, const uint32_t *all_lens, int *fits, int *value_bits, int *index_bits)
{
    return guarded(ctx, [&](Ctx &c) {
        ELBA_REQUIRE(fits, ELBA_ERR_INVALID_ARG, "dist_packed_format: null output");
        *fits = stage_dist_packed_format(c, nranks, read_bounds, all_lens, value_bits, index_bits) ? 1 : 0;
    });
}

int elba_dist_fill_send_packed(elba_ctx *ctx, int nranks, void *d_send, const uint64_t *offsets)
{
    return guarded(ctx, [&](Ctx &c) {
        ELBA_REQUIRE(offsets && (d_send || c.I == 0), ELBA_ERR_INVALID_ARG, "dist_fill_send_packed: null argument");
        stage_dist_fill_send_packed(c, nranks, d_send, offsets);
    });
}

int elba_dist_unpack_records(elba_ctx *ctx, int nranks, int rank, const void *d_packed, const uint64_t *recv_counts, void *d_records)
{
    return guarded(ctx, [&](Ctx &c) {
        ELBA_REQUIRE(recv_counts, ELBA_ERR_INVALID_ARG, "dist_unpack_records: null counts");
        stage_dist_unpack_records(c, nranks, rank, d_packed, recv_counts, d_records);
    });
}

int elba_dist_count_records(elba_ctx *ctx, const void *d_records, int64_t nrecords, elba_kmer_stats *stats)
{
    return guarded(ctx, [&](Ctx &c) {
        stage_dist_count_records(c, d_records, nrecords);
        if (stats) *stats = c.kstats;
    });
}

int elba_dist_get_reliable_kmers(elba_ctx *ctx, const void **d_kmers, int64_t *n)
{
    return guarded(ctx, [&](Ctx &c) {
        ELBA_REQUIRE(d_kmers && n, ELBA_ERR_INVALID_ARG, "dist_get_reliable_kmers: null output");
        ELBA_REQUIRE(has(c.v, P_COUNTS) && c.dist_owner, ELBA_ERR_STATE, "dist_get_reliable_kmers: call dist_count_records first");
        ELBA_REQUIRE(c.cfg.k <= 31, ELBA_ERR_UNSUPPORTED, "dist_get_reliable_kmers: multi-word k-mers are handed out interleaved by elba_dist_copy_reliable_kmers");
        *d_kmers = c.rel_kmers.p; *n = c.own_N;
    });
}

int elba_dist_copy_reliable_kmers(elba_ctx *ctx, void *d_dst, int64_t capacity)
{
    return guarded(ctx, [&](Ctx &c) {
        ELBA_REQUIRE(has(c.v, P_COUNTS) && c.dist_owner, ELBA_ERR_STATE, "dist_copy_reliable_kmers: call dist_count_records first");
        ELBA_REQUIRE(capacity >= c.own_N && (d_dst || c.own_N == 0), ELBA_ERR_INVALID_ARG, "dist_copy_reliable_kmers: buffer too small");
        stage_dist_copy_reliable_kmers(c, d_dst);
    });
}

int elba_dist_set_global_kmers(elba_ctx *ctx, const void *d_all_kmers, int64_t nall)
{
    return guarded(ctx, [&](Ctx &c) { stage_dist_set_global_kmers(c, d_all_kmers, nall); });
}

int elba_dist_panel_counts(elba_ctx *ctx, int nranks, const uint64_t *read_bounds, uint64_t *counts)
{
    return guarded(ctx, [&](Ctx &c) {
        ELBA_REQUIRE(read_bounds && counts, ELBA_ERR_INVALID_ARG, "dist_panel_counts: null argument");
        stage_dist_panel(c, nranks, read_bounds, nullptr, nullptr, false, nullptr, counts);
    });
}

int elba_dist_panel_fill(elba_ctx *ctx, int nranks, const uint64_t *read_bounds, void *d_send, const uint64_t *offsets)
{
    return guarded(ctx, [&](Ctx &c) {
        ELBA_REQUIRE(read_bounds && offsets, ELBA_ERR_INVALID_ARG, "dist_panel_fill: null argument");
        stage_dist_panel(c, nranks, read_bounds, nullptr, nullptr, true, d_send, const_cast<uint64_t *>(offsets));
    });
}

int elba_dist_panel_counts_win(elba_ctx *ctx, int nranks, const uint64_t *read_bounds, const uint64_t *win_lo, const uint64_t *win_hi, uint64_t *counts)
{
    return guarded(ctx, [&](Ctx &c) {
        ELBA_REQUIRE(read_bounds && win_lo && win_hi && counts, ELBA_ERR_INVALID_ARG, "dist_panel_counts_win: null argument");
        stage_dist_panel(c, nranks, read_bounds, win_lo, win_hi, false, nullptr, counts);
    });
}

int elba_dist_panel_fill_win(elba_ctx *ctx, int nranks, const uint64_t *read_bounds, const uint64_t *win_lo, const uint64_t *win_hi, void *d_send, const uint64_t *offsets)
{
    return guarded(ctx, [&](Ctx &c) {
        ELBA_REQUIRE(read_bounds && win_lo && win_hi && offsets, ELBA_ERR_INVALID_ARG, "dist_panel_fill_win: null argument");
        stage_dist_panel(c, nranks, read_bounds, win_lo, win_hi, true, d_send, const_cast<uint64_t *>(offsets));
    });
}

int elba_dist_set_panel(elba_ctx *ctx, const void *d_records, int64_t nrecords, int64_t nreads_total, int64_t nkmers_total, int64_t row_lo, int64_t row_hi, elba_matrix_stats *stats)
{
    return guarded(ctx, [&](Ctx &c) {
        EventTimer t;
        t.start(c.stream);
        stage_dist_set_panel(c, d_records, nrecords, nreads_total, nkmers_total, row_lo, row_hi);
        t.stop(c.stream);
        if (stats) { stats->nrows = c.M; stats->ncols = c.N_global >= 0 ? c.N_global : c.N; stats->nnz = c.Z; stats->max_row_nnz = c.max_row_nnz; stats->ms_total = t.ms(); }
    });
}

}  // extern "C"
