// text_index.hip — raw FASTA / FASTQ text -> the .fai records of its reads, on the device.
//
// elba_set_reads_fasta needs (len, pos, bases) of every read and leaves finding them to the host (fasta.write_fai: a per-line loop).  Here
// the index is built where the chunk already is: newline ranks give the line starts, header flags give the records, and every field of a
// record is a closed form of line starts.  The existing k_fasta_encode (ingest.hip) then runs on records that never left the device.
//
//   pass 1  k_text_count   one 16-byte load per lane, TEXT_TILE_BYTES per workgroup: '\n' per tile (__ballot / __popcll), line-start '>'
//                          in all, the first '\r'
//           scan           tile counts -> the rank of every tile's first newline
//   pass 2  k_text_lines   the same loads again: line_start[rank + 1] = offset + 1 of every newline
//   FASTA   k_fa_flags, scan, k_fa_scatter (record -> header line), k_fa_shape (one lane per line), k_fa_records (one lane per record)
//   FASTQ   k_fq_records   (one lane per record: five line starts)
//           k_text_names, scan of (len + 3) / 4 -> byte_off
//
// Side arrays are per tile, per line and per record, never per byte.  Every index a kernel forms is bounded by a count an earlier pass
// produced and the host read back (lines, records), and every violation of the grammar goes through one 64-bit atomicMin of
// offset << 3 | kind, so the violation with the smallest file offset is the one reported whatever the order the lanes ran in.
#include "common.hpp"

namespace elba {

namespace {

constexpr uint32_t TX_THREADS = 256;
static_assert(TEXT_TILE_BYTES == 16 * TX_THREADS, "one 16-byte load per lane and tile");

// kinds of a violation: the low three bits of the error word (on one offset the smaller kind is reported)
enum : uint32_t { TXE_CR = 0, TXE_FIRST = 1, TXE_SHAPE = 2, TXE_FQ_LINES = 3, TXE_FQ_AT = 4, TXE_FQ_PLUS = 5, TXE_FQ_QUAL = 6, TXE_LONG = 7 };
const char *const TXE_TEXT[8] = {
    "carriage return", "first byte is neither '>' nor '@'", "sequence line breaks the line shape bases, .., bases, t, 0, .., 0",
    "FASTQ line count is no multiple of 4", "FASTQ record does not start with '@'", "FASTQ separator line does not start with '+'",
    "FASTQ quality line and sequence line differ in length", "read of 0x7FFFFFF0 bases or more"};
constexpr unsigned long long TX_NO_ERROR = ~0ull;

struct TxCtr { unsigned long long err, nhdr; };

__device__ __forceinline__ void tx_error(TxCtr *ctr, uint64_t file_offset, uint32_t kind) { atomicMin(&ctr->err, (unsigned long long)(file_offset << 3 | kind)); }

// the 16 bytes of the chunk at `off` (a multiple of 16; the chunk's buffer is 16-byte aligned); zero beyond its end
__device__ __forceinline__ uint4 tx_load16(const uint8_t *chunk, uint64_t n, uint64_t off)
{
    uint4 v = make_uint4(0u, 0u, 0u, 0u);
    if (off + 16 <= n) v = *reinterpret_cast<const uint4 *>(chunk + off);
    else for (uint32_t q = 0; q < 16 && off + q < n; ++q) reinterpret_cast<uint8_t *>(&v)[q] = chunk[off + q];
    return v;
}

// bit j of the result: byte j of v equals c
__device__ __forceinline__ uint32_t tx_match16(const uint4 &v, uint32_t c)
{
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
    uint32_t m = 0;
#pragma unroll
    for (int j = 0; j < 16; ++j) m |= (((w[j >> 2] >> (8 * (j & 3))) & 0xFFu) == c ? 1u : 0u) << j;
    return m;
}

// Pass 1.  tile_cnt[t] = newlines of tile t (tile_cnt[ntiles] = 0: the scan's last element is the total); ctr->nhdr += '>' at a line
// start (offset 0, or behind a '\n'): the FASTA record count, known before any per-record array is sized; ctr->err: the first '\r'.
__global__ __launch_bounds__(TX_THREADS) void k_text_count(const uint8_t *chunk, uint64_t n, uint64_t file_off, uint64_t ntiles, uint32_t *tile_cnt, TxCtr *ctr)
{
    __shared__ uint32_t s_nl[TX_THREADS / 64], s_hd[TX_THREADS / 64];
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    unsigned long long headers = 0;
    if (blockIdx.x == 0 && threadIdx.x == 0) tile_cnt[ntiles] = 0;
    for (uint64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const uint64_t off = t * TEXT_TILE_BYTES + 16ull * threadIdx.x;
        const uint4 v = tx_load16(chunk, n, off);
        const uint32_t nl = tx_match16(v, '\n'), cr = tx_match16(v, '\r'), gt = tx_match16(v, '>');
        // does this lane's first byte begin a line?  The byte before it is the last one of the lane below; a wave's first lane reads it
        uint32_t prev_nl = (uint32_t)__shfl_up((int)(nl >> 15), 1, 64);
        if (lane == 0) prev_nl = off == 0 ? 1u : (off - 1 < n && chunk[off - 1] == '\n' ? 1u : 0u);
        const uint32_t hd = gt & ((nl << 1 | prev_nl) & 0xFFFFu);
        uint32_t wnl = 0, whd = 0;
#pragma unroll
        for (int j = 0; j < 16; ++j) wnl += (uint32_t)__popcll(__ballot((nl >> j) & 1u));
        if (__ballot(hd != 0)) {
#pragma unroll
            for (int j = 0; j < 16; ++j) whd += (uint32_t)__popcll(__ballot((hd >> j) & 1u));
        }
        const unsigned long long crm = __ballot(cr != 0);
        if (crm && lane == (uint32_t)__ffsll((long long)crm) - 1u) tx_error(ctr, file_off + off + (uint32_t)(__ffs((int)cr) - 1), TXE_CR);      // lanes ascend with the offset
        if (lane == 0) { s_nl[wave] = wnl; s_hd[wave] = whd; }
        __syncthreads();
        if (threadIdx.x == 0) {
            uint32_t a = 0, b = 0;
            for (uint32_t w = 0; w < TX_THREADS / 64; ++w) { a += s_nl[w]; b += s_hd[w]; }
            tile_cnt[t] = a; headers += b;
        }
        __syncthreads();
    }
    if (threadIdx.x == 0 && headers) atomicAdd(&ctr->nhdr, headers);
}

// Pass 2.  line_start[k + 1] = offset + 1 of the newline of rank k; line_start[0] = 0; line_start[nlines] = n + 1 when the chunk does
// not end in a newline, so that line i is [line_start[i], line_start[i + 1] - 1) for every i < nlines.
__global__ __launch_bounds__(TX_THREADS) void k_text_lines(const uint8_t *chunk, uint64_t n, uint64_t ntiles, const int64_t *tile_base, uint64_t nlines, uint32_t final_nl, uint64_t *line_start)
{
    __shared__ uint32_t s_w[TX_THREADS / 64];
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (blockIdx.x == 0 && threadIdx.x == 0) { line_start[0] = 0; if (!final_nl) line_start[nlines] = n + 1; }
    for (uint64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const uint64_t off = t * TEXT_TILE_BYTES + 16ull * threadIdx.x;
        const uint4 v = tx_load16(chunk, n, off);
        uint32_t nl = tx_match16(v, '\n');
        const uint32_t cnt = (uint32_t)__popc(nl);
        uint32_t inc = cnt;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) { const uint32_t o = (uint32_t)__shfl_up((int)inc, d, 64); if (lane >= (uint32_t)d) inc += o; }
        if (lane == 63) s_w[wave] = inc;
        __syncthreads();
        uint64_t rank = (uint64_t)tile_base[t] + inc - cnt;
        for (uint32_t w = 0; w < wave; ++w) rank += s_w[w];
        while (nl) {
            const uint32_t j = (uint32_t)__ffs((int)nl) - 1u;
            nl &= nl - 1u;
            if (rank + 1 <= nlines) line_start[rank + 1] = off + j + 1;
            ++rank;
        }
        __syncthreads();
    }
}

__device__ __forceinline__ uint64_t tx_line_len(const uint64_t *line_start, uint64_t i) { return line_start[i + 1] - 1 - line_start[i]; }      // (i < nlines)

// hdr[i] = line i begins with '>' (hdr[nlines] = 0: the scan runs over nlines + 1 elements)
__global__ void k_fa_flags(const uint8_t *chunk, uint64_t n, const uint64_t *line_start, uint64_t nlines, uint32_t *hdr)
{
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i <= nlines; i += (uint64_t)gridDim.x * blockDim.x)
        hdr[i] = i < nlines && line_start[i] < n && chunk[line_start[i]] == '>' ? 1u : 0u;
}

// rec_line[r] = header line of record r (filled with nlines beforehand: rec_line[nrec] is the sentinel)
__global__ void k_fa_scatter(const uint32_t *hdr, const uint32_t *rol, uint64_t nlines, uint64_t nrec, uint32_t *rec_line)
{
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nlines; i += (uint64_t)gridDim.x * blockDim.x)
        if (hdr[i] && rol[i] < nrec) rec_line[rol[i]] = (uint32_t)i;
}

// The line lengths of a record read bases, .., bases, t, 0, .., 0 (0 <= t <= bases) exactly when every sequence line has l <= bases and
// (l == bases, or its successor in the record is empty, or it is the record's last line): a local rule, one lane per line.
__global__ void k_fa_shape(const uint64_t *line_start, const uint32_t *hdr, const uint32_t *rol, const uint32_t *rec_line, uint64_t nlines, uint64_t nrec, uint64_t file_off, TxCtr *ctr)
{
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nlines; i += (uint64_t)gridDim.x * blockDim.x) {
        if (hdr[i]) continue;
        const uint64_t before = rol[i];      // headers before line i
        if (before == 0) { if (i == 0) tx_error(ctr, file_off, TXE_FIRST); continue; }      // (lines in front of the first header: offset 0 is reported, nothing beats it)
        if (before > nrec) continue;
        const uint64_t h = rec_line[before - 1], next = rec_line[before];
        if (!(h < i && i < next && next <= nlines)) continue;
        const uint64_t bases = tx_line_len(line_start, h + 1), l = tx_line_len(line_start, i);
        const bool ok = l <= bases && (l == bases || i + 1 == next || tx_line_len(line_start, i + 1) == 0);
        if (!ok) tx_error(ctr, file_off + line_start[i], TXE_SHAPE);
    }
}

// record r from line ranks alone: pos behind the header's newline, len = end - pos - newlines in between, bases = the first line's length
__global__ void k_fa_records(const uint64_t *line_start, const uint32_t *rec_line, uint64_t nlines, uint64_t nrec, uint64_t n, uint32_t final_nl, uint64_t file_off,
                             elba_fasta_record_t *recs, uint32_t *lens, uint32_t *nb4, TxCtr *ctr)
{
    for (uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; r <= nrec; r += (uint64_t)gridDim.x * blockDim.x) {
        if (r == nrec) { nb4[r] = 0; continue; }
        const uint64_t h = rec_line[r], next = rec_line[r + 1];
        uint64_t len = 0, pos = n, bases = 1;
        if (h < next && next <= nlines) {
            const uint64_t end = line_start[next] < n ? line_start[next] : n, nseq = next - h - 1;
            pos = line_start[h + 1] < n ? line_start[h + 1] : n;
            len = end - pos - (nseq - (next == nlines && !final_nl && nseq ? 1 : 0));
            bases = nseq ? tx_line_len(line_start, h + 1) : 0;
            if (len == 0) bases = 1;
            if (len >= 0x7FFFFFF0ull) { tx_error(ctr, file_off + line_start[h], TXE_LONG); len = 0; }
        }
        recs[r].len = len; recs[r].pos = file_off + pos; recs[r].bases = bases;
        lens[r] = (uint32_t)len; nb4[r] = (uint32_t)((len + 3) / 4);
    }
}

// FASTQ: record r is the lines 4r .. 4r + 3; the rank of a line decides its role, not its first character
__global__ void k_fq_records(const uint8_t *chunk, const uint64_t *line_start, uint64_t nlines, uint64_t nrec, uint64_t n, uint64_t file_off,
                             elba_fasta_record_t *recs, uint32_t *lens, uint32_t *nb4, TxCtr *ctr)
{
    for (uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; r <= nrec; r += (uint64_t)gridDim.x * blockDim.x) {
        if (r == nrec) {
            nb4[r] = 0;
            if (nlines != 4 * nrec) tx_error(ctr, file_off + line_start[4 * nrec], TXE_FQ_LINES);      // the first line of the incomplete record
            continue;
        }
        const uint64_t s0 = line_start[4 * r], s1 = line_start[4 * r + 1], s2 = line_start[4 * r + 2], s3 = line_start[4 * r + 3], s4 = line_start[4 * r + 4];
        uint64_t len = s2 - 1 - s1;
        if (!(s0 < n && chunk[s0] == '@')) tx_error(ctr, file_off + s0, TXE_FQ_AT);
        if (!(s2 < n && chunk[s2] == '+')) tx_error(ctr, file_off + s2, TXE_FQ_PLUS);
        if (s4 - 1 - s3 != len) tx_error(ctr, file_off + s0, TXE_FQ_QUAL);
        if (len >= 0x7FFFFFF0ull) { tx_error(ctr, file_off + s0, TXE_LONG); len = 0; }
        recs[r].len = len; recs[r].pos = file_off + s1; recs[r].bases = len ? len : 1;
        lens[r] = (uint32_t)len; nb4[r] = (uint32_t)((len + 3) / 4);
    }
}

// the name: behind the '>' / '@' up to the first space, tab, VT or FF, or the line's end (what bytes.split()[0] yields); it may be empty
__global__ void k_text_names(const uint8_t *chunk, const uint64_t *line_start, const uint32_t *rec_line /* null: FASTQ */, uint64_t nlines, uint64_t nrec, uint64_t n, uint64_t file_off,
                             uint64_t *name_pos, uint32_t *name_len)
{
    for (uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; r < nrec; r += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t h = rec_line ? rec_line[r] : 4 * r;
        uint64_t p = n, q = n;
        if (h < nlines) {
            uint64_t e = line_start[h + 1] - 1;
            if (e > n) e = n;
            p = line_start[h] + 1 < e ? line_start[h] + 1 : e;
            for (q = p; q < e; ++q) { const uint8_t ch = chunk[q]; if (ch == ' ' || ch == '\t' || ch == '\v' || ch == '\f') break; }
        }
        name_pos[r] = file_off + p; name_len[r] = (uint32_t)(q - p);
    }
}

unsigned grid_for(const Ctx &c, uint64_t items, uint32_t threads)
{
    const uint64_t want = (items + threads - 1) / threads, cap = (uint64_t)c.num_cus * 8;
    return (unsigned)(want < 1 ? 1 : (want < cap ? want : cap));
}

// the record a violation lies in, for the message (the rejected path only: a walk over the host's copy of the chunk up to the offset)
int64_t record_of_offset(const char *chunk, uint64_t rel, bool fasta)
{
    int64_t headers = 0, newlines = 0;
    for (uint64_t i = 0; i <= rel; ++i) {
        if (fasta && chunk[i] == '>' && (i == 0 || chunk[i - 1] == '\n')) ++headers;
        if (i < rel && chunk[i] == '\n') ++newlines;
    }
    return fasta ? (headers > 0 ? headers - 1 : 0) : newlines / 4;
}

}  // namespace

void stage_set_reads_text(Ctx &c, const char *chunk, int64_t chunk_bytes, uint64_t chunk_file_offset, const elba_text_cfg *cfg, elba_text_stats *stats)
{
    enter(c.v, EV_SET_READS_FASTA);
    ELBA_REQUIRE(chunk_bytes >= 0 && (chunk_bytes == 0 || chunk), ELBA_ERR_INVALID_ARG, "set_reads_text: null chunk");
    int format = cfg ? cfg->format : ELBA_TEXT_AUTO;
    const int64_t first_global_id = cfg ? cfg->first_global_id : 0;
    ELBA_REQUIRE(format >= ELBA_TEXT_AUTO && format <= ELBA_TEXT_FASTQ && (!cfg || cfg->flags == 0), ELBA_ERR_INVALID_ARG, "set_reads_text: unknown format or non-zero flags");
    const uint64_t n = (uint64_t)chunk_bytes;
    if (format == ELBA_TEXT_AUTO) {
        if (n == 0 || chunk[0] == '>') format = ELBA_TEXT_FASTA;
        else if (chunk[0] == '@') format = ELBA_TEXT_FASTQ;
        else {
            const uint32_t kind = chunk[0] == '\r' ? TXE_CR : TXE_FIRST;
            throw Error{ELBA_ERR_INVALID_ARG, std::string("set_reads_text: ") + TXE_TEXT[kind] + " (kind " + std::to_string(kind) + ") in record 0 at file offset " + std::to_string(chunk_file_offset)};
        }
    }
    const bool fasta = format == ELBA_TEXT_FASTA;
    const uint32_t final_nl = n && chunk[n - 1] == '\n' ? 1u : 0u;
    const uint64_t ntiles = (n + TEXT_TILE_BYTES - 1) / TEXT_TILE_BYTES;
    hipStream_t s = c.stream;

    // scratch of this call (the chunk's size or per line: given back when the call returns) and the new read set's arrays, which take
    // the place of the context's only when the call has succeeded — a rejected call leaves the previous reads and their index alone
    DevBuf d_chunk, d_tile_cnt, d_tile_base, d_ctr, d_ls, d_hdr, d_rol, d_rec_line, d_nb4;
    DevBuf n_recs, n_name_pos, n_name_len, n_len, n_boff;
    d_chunk.reserve((size_t)n + 16); d_tile_cnt.reserve((size_t)(ntiles + 1) * 4); d_tile_base.reserve((size_t)(ntiles + 1) * 8); d_ctr.reserve(sizeof(TxCtr));
    c.t_total.start(s);
    if (n) ELBA_HIP(hipMemcpyAsync(d_chunk.p, chunk, (size_t)n, hipMemcpyHostToDevice, s));
    const TxCtr ctr0{TX_NO_ERROR, 0};
    ELBA_HIP(hipMemcpyAsync(d_ctr.p, &ctr0, sizeof(ctr0), hipMemcpyHostToDevice, s));
    c.t_b.start(s);
    uint64_t nlines = 0, nrec = 0;
    if (n) {
        hipLaunchKernelGGL(k_text_count, dim3(grid_for(c, ntiles, 1)), dim3(TX_THREADS), 0, s, d_chunk.as<uint8_t>(), n, chunk_file_offset, ntiles, d_tile_cnt.as<uint32_t>(), d_ctr.as<TxCtr>());
        ELBA_HIP(hipGetLastError());
        exclusive_scan_u32_to_i64(s, d_tile_cnt.as<uint32_t>(), d_tile_base.as<int64_t>(), (int64_t)ntiles + 1, c.ws_scan);
        // first read-back: the newlines and the line-start '>' of the whole chunk — what sizes the per-line and per-record arrays
        TxCtr h_ctr{}; int64_t newlines = 0;
        ELBA_HIP(hipMemcpyAsync(&h_ctr, d_ctr.p, sizeof(h_ctr), hipMemcpyDeviceToHost, s));
        ELBA_HIP(hipMemcpyAsync(&newlines, d_tile_base.as<int64_t>() + ntiles, 8, hipMemcpyDeviceToHost, s));
        ELBA_HIP(hipStreamSynchronize(s));
        nlines = (uint64_t)newlines + (final_nl ? 0 : 1);
        nrec = fasta ? h_ctr.nhdr : nlines / 4;
        ELBA_REQUIRE(nlines < 0xFFFFFFFFull && nrec < 0xFFFFFFFFull, ELBA_ERR_UNSUPPORTED, "set_reads_text: more than 2^32-1 lines or reads on one GPU");
    }
    d_ls.reserve((size_t)(nlines + 2) * 8); d_nb4.reserve((size_t)(nrec + 1) * 4);
    if (fasta) { d_hdr.reserve((size_t)(nlines + 1) * 4); d_rol.reserve((size_t)(nlines + 1) * 4); d_rec_line.reserve((size_t)(nrec + 1) * 4); }
    n_recs.reserve((size_t)(nrec + 1) * sizeof(elba_fasta_record_t)); n_name_pos.reserve((size_t)(nrec + 1) * 8); n_name_len.reserve((size_t)(nrec + 1) * 4);
    n_len.reserve((size_t)(nrec + 1) * 4); n_boff.reserve((size_t)(nrec + 1) * 8);
    uint64_t *ls = d_ls.as<uint64_t>();
    elba_fasta_record_t *recs = n_recs.as<elba_fasta_record_t>();
    unsigned long long err = TX_NO_ERROR;
    int64_t pb = 0;
    if (n) {
        hipLaunchKernelGGL(k_text_lines, dim3(grid_for(c, ntiles, 1)), dim3(TX_THREADS), 0, s, d_chunk.as<uint8_t>(), n, ntiles, d_tile_base.as<int64_t>(), nlines, final_nl, ls);
        if (fasta) {
            uint32_t *hdr = d_hdr.as<uint32_t>(), *rol = d_rol.as<uint32_t>(), *rec_line = d_rec_line.as<uint32_t>();
            hipLaunchKernelGGL(k_fa_flags, dim3(grid_for(c, nlines + 1, 256)), dim3(256), 0, s, d_chunk.as<uint8_t>(), n, ls, nlines, hdr);
            exclusive_scan_u32(s, hdr, rol, (int64_t)nlines + 1, c.ws_scan);
            fill_u32(s, rec_line, (uint32_t)nlines, (int64_t)nrec + 1);
            hipLaunchKernelGGL(k_fa_scatter, dim3(grid_for(c, nlines, 256)), dim3(256), 0, s, hdr, rol, nlines, nrec, rec_line);
            hipLaunchKernelGGL(k_fa_shape, dim3(grid_for(c, nlines, 256)), dim3(256), 0, s, ls, hdr, rol, rec_line, nlines, nrec, chunk_file_offset, d_ctr.as<TxCtr>());
            hipLaunchKernelGGL(k_fa_records, dim3(grid_for(c, nrec + 1, 256)), dim3(256), 0, s, ls, rec_line, nlines, nrec, n, final_nl, chunk_file_offset, recs, n_len.as<uint32_t>(),
                               d_nb4.as<uint32_t>(), d_ctr.as<TxCtr>());
        } else {
            hipLaunchKernelGGL(k_fq_records, dim3(grid_for(c, nrec + 1, 256)), dim3(256), 0, s, d_chunk.as<uint8_t>(), ls, nlines, nrec, n, chunk_file_offset, recs, n_len.as<uint32_t>(),
                               d_nb4.as<uint32_t>(), d_ctr.as<TxCtr>());
        }
        if (nrec)
            hipLaunchKernelGGL(k_text_names, dim3(grid_for(c, nrec, 256)), dim3(256), 0, s, d_chunk.as<uint8_t>(), ls, fasta ? d_rec_line.as<uint32_t>() : (const uint32_t *)nullptr, nlines, nrec, n,
                               chunk_file_offset, n_name_pos.as<uint64_t>(), n_name_len.as<uint32_t>());
        ELBA_HIP(hipGetLastError());
        exclusive_scan_u32_to_i64(s, d_nb4.as<uint32_t>(), n_boff.as<int64_t>(), (int64_t)nrec + 1, c.ws_scan);
        c.t_b.stop(s);
        // second read-back: the error word and the packed size
        ELBA_HIP(hipMemcpyAsync(&err, d_ctr.p, 8, hipMemcpyDeviceToHost, s));
        ELBA_HIP(hipMemcpyAsync(&pb, n_boff.as<int64_t>() + nrec, 8, hipMemcpyDeviceToHost, s));
        ELBA_HIP(hipStreamSynchronize(s));
    } else {
        c.t_b.stop(s);
        ELBA_HIP(hipMemsetAsync(n_boff.p, 0, 8, s));
    }
    if (err != TX_NO_ERROR) {
        const uint32_t kind = (uint32_t)(err & 7u);
        const uint64_t off = err >> 3;
        const int64_t rec = kind == TXE_FIRST ? 0 : record_of_offset(chunk, off - chunk_file_offset < n ? off - chunk_file_offset : n - 1, fasta);
        throw Error{ELBA_ERR_INVALID_ARG, std::string("set_reads_text: ") + TXE_TEXT[kind] + " (kind " + std::to_string(kind) + ") in record " + std::to_string(rec) + " at file offset " + std::to_string(off)};
    }
    accepted(c.v, EV_SET_READS_FASTA);
    c.own_packed.reserve((size_t)pb + 16);          // +16: the enumerate kernel reads whole 8-byte windows
    ELBA_HIP(hipMemsetAsync(c.own_packed.p, 0, (size_t)pb + 16, s));
    c.t_a.start(s);
    if (nrec) launch_fasta_encode(c, d_chunk.as<uint8_t>(), chunk_file_offset, n, recs, n_boff.as<uint64_t>(), (int64_t)nrec, c.own_packed.as<uint8_t>());
    c.t_a.stop(s);
    std::vector<elba_fasta_record_t> h_recs((size_t)nrec);
    std::vector<uint64_t> h_name_pos((size_t)nrec), h_boff((size_t)nrec);
    std::vector<uint32_t> h_name_len((size_t)nrec), h_len((size_t)nrec);
    if (nrec) {
        ELBA_HIP(hipMemcpyAsync(h_recs.data(), n_recs.p, (size_t)nrec * sizeof(elba_fasta_record_t), hipMemcpyDeviceToHost, s));
        ELBA_HIP(hipMemcpyAsync(h_name_pos.data(), n_name_pos.p, (size_t)nrec * 8, hipMemcpyDeviceToHost, s));
        ELBA_HIP(hipMemcpyAsync(h_name_len.data(), n_name_len.p, (size_t)nrec * 4, hipMemcpyDeviceToHost, s));
        ELBA_HIP(hipMemcpyAsync(h_len.data(), n_len.p, (size_t)nrec * 4, hipMemcpyDeviceToHost, s));
        ELBA_HIP(hipMemcpyAsync(h_boff.data(), n_boff.p, (size_t)nrec * 8, hipMemcpyDeviceToHost, s));
    }
    c.t_total.stop(s);
    ELBA_HIP(hipStreamSynchronize(s));
    // the new arrays become the context's (the old ones leave with this call's scratch)
    c.own_byte_off.swap(n_boff); c.own_len.swap(n_len);
    c.tx_recs.swap(n_recs); c.tx_name_pos.swap(n_name_pos); c.tx_name_len.swap(n_name_len);
    c.d_packed = c.own_packed.as<uint8_t>(); c.d_byte_off = c.own_byte_off.as<uint64_t>(); c.d_len = c.own_len.as<uint32_t>();
    uint64_t totbases = 0;
    for (uint32_t l : h_len) totbases += l;
    c.h_len.swap(h_len); c.h_byte_off.swap(h_boff);
    c.tx_h_recs.swap(h_recs); c.tx_h_name_pos.swap(h_name_pos); c.tx_h_name_len.swap(h_name_len);
    c.nreads = (int64_t)nrec; c.first_global_id = first_global_id; c.packed_bytes = pb;
    reads_replaced(c, EV_SET_READS_FASTA);
    c.tx_index = true;      // (reads_replaced forgot the previous read set's index)
    if (stats) {
        stats->nreads = (int64_t)nrec; stats->bases = (int64_t)totbases; stats->packed_bytes = pb; stats->chunk_bytes = chunk_bytes; stats->lines = (int64_t)nlines;
        stats->format = format; stats->reserved = 0;
        stats->ms_total = c.t_total.ms(); stats->ms_index = c.t_b.ms(); stats->ms_encode = nrec ? c.t_a.ms() : 0.f;
    }
}

void stage_export_read_index(Ctx &c, elba_fasta_record_t *recs, uint64_t *name_pos, uint32_t *name_len, int64_t nreads_capacity)
{
    ELBA_REQUIRE(has(c.v, P_READS) && c.tx_index, ELBA_ERR_STATE, "export_read_index: the context's reads do not come from elba_set_reads_text");
    ELBA_REQUIRE(nreads_capacity >= c.nreads, ELBA_ERR_INVALID_ARG, "export_read_index: arrays too small");
    const size_t m = (size_t)c.nreads;
    if (recs && m) memcpy(recs, c.tx_h_recs.data(), m * sizeof(elba_fasta_record_t));
    if (name_pos && m) memcpy(name_pos, c.tx_h_name_pos.data(), m * 8);
    if (name_len && m) memcpy(name_len, c.tx_h_name_len.data(), m * 4);
}

}  // namespace elba
