// matrix.hip — device construction of A in both orientations.
//   CSC(A)  = the reference's AT (src/main.cpp:272-273): column k-mer, entries (read, pos) ordered by (read, pos)
//   CSR(A)  = the reference's A  (src/KmerOps.cpp:361-401): row read, entries (kid, pos) ordered by (kid, pos)
// Entries are single u64 words (hi = read or kid, lo = pos) so that one 8-byte load fetches an entry and a row /
// column segment sorted as u64 is in canonical order.  Duplicate (read,kid) entries are kept (SumDuplicates=false,
// src/KmerOps.cpp:400).  A CSR entry also carries two ownership bits above its position (Ctx::csr_hints, common.hpp), and the columns
// exist a second time padded to a common stride (a_ell): the store the SpGEMM fetches from.
#include "common.hpp"
#include "matrix.hpp"
#include <algorithm>

namespace elba {

namespace {

// hint bits of entry z (read i) from its column, and the column's length added to the window's product count (one atomic per wavefront)
__device__ __forceinline__ uint32_t entry_hint(const uint32_t *colptr, const uint64_t *csc, uint64_t kid, uint32_t i, bool hints, uint32_t win_lo, uint32_t win_hi, unsigned long long *prod_ctr)
{
    const uint32_t c0 = colptr[kid], L = colptr[kid + 1] - c0;
    unsigned long long mine = i >= win_lo && i < win_hi ? L : 0u;
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) mine += __shfl_xor(mine, d, 64);
    if ((threadIdx.x & 63) == 0 && mine) atomicAdd(&prod_ctr[(blockIdx.x & 63u) * 16u], mine);      // (64 counters on lines of their own)
    return hints && L <= HINT_MAX_COL ? column_hint(csc + c0, L, i, win_lo, win_hi) : 0u;
}

__global__ void k_csc_to_csr_keys(const uint64_t *kid_keys, int kid_shift, uint64_t kid_mask, const uint32_t *colptr, const uint64_t *csc, int64_t Z, uint32_t *row_keys, uint64_t *csr_vals,
                                  bool hints, bool suffix, uint32_t win_lo, uint32_t win_hi, unsigned long long *prod_ctr, const uint8_t *colw0)
{
    int64_t z = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const bool in = z < Z;
    if (!in) z = Z - 1;                                      // (whole wavefronts reach the reduction inside entry_hint)
    uint64_t kid = (kid_keys[z] >> kid_shift) & kid_mask;
    uint64_t e = csc[z];
    const uint32_t h = entry_hint(colptr, csc, kid, in ? (uint32_t)(e >> 32) : 0xFFFFFFFFu, hints && in, in ? win_lo : 0u, in ? win_hi : 0u, prod_ctr);
    if (!in) return;
    row_keys[z] = (uint32_t)(e >> 32);                       // read
    if (suffix) {      // dense matrices (Ctx::csr_suffix): the entry knows its column's length and its own place in it — kid | L << 23 | idx << 16 | pos (16 bits)
        const uint32_t c0 = colptr[kid], L = colptr[kid + 1] - c0;
        uint32_t idx = (uint32_t)z - c0;
        if (colw0) { const uint32_t w0 = colw0[kid]; idx = idx >= w0 ? idx - w0 : idx + L - w0; }      // (a row window: the padded column is stored rotated, see k_fill_ell)
        csr_vals[z] = (kid << 32) | ((uint64_t)L << 23) | ((uint64_t)idx << 16) | (e & 0xFFFFull);
    } else csr_vals[z] = (kid << 32) | ((uint64_t)h << 30) | (e & 0xFFFFFFFFull);         // kid | hint | pos
}

// CSR build with ONE word per entry when read, k-mer id, the two hint bits and the position fit 64 bits together:
// read << (nb + pb + 2) | kid << (pb + 2) | hint << pb | pos, sorted on the read bits only (stable: rows come out in (kid, pos) order)
__global__ void k_csc_to_csr_words(const uint64_t *kid_keys, int kid_shift, const uint32_t *colptr, const uint64_t *csc, int64_t Z, int nb, int pb, int rs, int pbi, uint64_t *words,
                                   bool hints, uint32_t win_lo, uint32_t win_hi, unsigned long long *prod_ctr)
{
    int64_t z = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const bool in = z < Z;
    if (!in) z = Z - 1;
    const uint64_t kid = kid_keys[z] >> kid_shift, e = csc[z];
    const uint32_t h = entry_hint(colptr, csc, kid, in ? (uint32_t)(e >> 32) : 0xFFFFFFFFu, hints && in, in ? win_lo : 0u, in ? win_hi : 0u, prod_ctr);
    if (!in) return;
    uint64_t word = ((e >> 32) << rs) | (kid << (pb + 2)) | ((uint64_t)h << pb) | (e & 0xFFFFFFFFull);
    if (pbi) {
        // Ctx::csr_inline, as kmer_msd.hip writes it: a row that accumulates exactly ONE pair of this column under the parity rule over ALL rows
        // carries that pair in its own entry — flag | read << rs | (partner >> 1) << 2 pbi | posQ << pbi | posT — when both positions fit pbi bits
        const uint32_t c0 = colptr[kid], L = colptr[kid + 1] - c0, i = (uint32_t)(e >> 32);
        if (L <= HINT_MAX_COL) {
            uint32_t nown = 0, mult = 0;
            uint64_t other = 0;
            for (uint32_t t = 0; t < L; ++t) {
                const uint64_t y = csc[c0 + t];
                const uint32_t j = (uint32_t)(y >> 32);
                if (j == i) { ++mult; continue; }
                if (((i ^ j) & 1u) ? j < i : j > i) { ++nown; other = y; }
            }
            const uint64_t pos = e & 0xFFFFFFFFull, opos = other & 0xFFFFFFFFull;
            if (mult == 1u && nown == 1u && ((pos | opos) >> pbi) == 0)
                word = csr_inline_word(e >> 32, rs, other >> 32, pbi, pos, opos);
        }
    }
    words[z] = word;
}
// hint bits for sort keys that came without them (k_runs_emit, kmer.hip): the entry's k-mer id is in the word, its column in the CSC
// (one lane per entry; one lane per COLUMN, its entries in registers, was measured: 7.0 ms against 5.2)
__global__ void k_add_hints(const uint32_t *colptr, const uint64_t *csc, int64_t Z, int nb, int pb, int rs, int pbi, uint64_t *words)
{
    const int64_t z = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (z >= Z) return;
    const uint64_t w = words[z];
    const uint64_t kid = (w >> (pb + 2)) & ((1ull << nb) - 1);
    const uint32_t c0 = colptr[kid], L = colptr[kid + 1] - c0;
    if (L > HINT_MAX_COL) return;
    const uint64_t e = csc[z];
    const uint32_t i = (uint32_t)(e >> 32);
    if (pbi) {
        // Ctx::csr_inline (the whole matrix, parity rule over all rows): exactly one pair of this column accumulated by this row -> the entry carries it
        uint32_t nown = 0, mult = 0;
        uint64_t other = 0;
        for (uint32_t t = 0; t < L; ++t) {
            const uint64_t y = csc[c0 + t];
            const uint32_t j = (uint32_t)(y >> 32);
            if (j == i) { ++mult; continue; }
            if (((i ^ j) & 1u) ? j < i : j > i) { ++nown; other = y; }
        }
        const uint64_t pos = e & 0xFFFFFFFFull, opos = other & 0xFFFFFFFFull;
        if (mult == 1u && nown == 1u && ((pos | opos) >> pbi) == 0) { words[z] = csr_inline_word(e >> 32, rs, other >> 32, pbi, pos, opos); return; }
        if (mult < 2u && nown == 0u) words[z] = w | (3ull << pb);      // (the whole matrix: both hint bits agree)
        return;
    }
    words[z] = w | ((uint64_t)column_hint(csc + c0, L, i, 0u, 0xFFFFFFFFu) << pb);      // (the window is the whole matrix)
}
// sorted keys -> CSR entries, and the row pointers with them: entry z opens the rows (read of z - 1, read of z]; launched with Z + 1 lanes,
// the last of which closes the rows behind the last entry
__global__ void k_unpack_csr_words(const uint64_t *words, int64_t Z, int nb, int pb, int rs, int mb, int pbi, uint64_t *csr, uint32_t *rowptr, int64_t M)
{
    int64_t z = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (z > Z) return;
    const uint64_t rmask = (1ull << mb) - 1;
    const int64_t prev = z == 0 ? -1 : (int64_t)((words[z - 1] >> rs) & rmask);
    const uint64_t w = z < Z ? words[z] : 0;
    const int64_t cur = z < Z ? (int64_t)((w >> rs) & rmask) : M;
    for (int64_t k = prev + 1; k <= cur; ++k) rowptr[k] = (uint32_t)z;
    if (z < Z) csr[z] = csr_entry_of_word(w, nb, pb, mb, pbi);      // (an inline partner, Ctx::csr_inline, or kid | hint | pos: csr_plan.hpp)
}

__global__ void k_colrow_to_csc(const uint64_t *colrow, const uint64_t *pos, int64_t Z, uint64_t *csc)
{
    int64_t z = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (z >= Z) return;
    csc[z] = ((colrow[z] & 0xFFFFFFFFull) << 32) | (pos[z] & 0xFFFFFFFFull);
}

__global__ void k_max_seg_len(const uint32_t *ptr, int64_t nseg, unsigned long long *out)
{
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    int64_t stride = (int64_t)gridDim.x * blockDim.x;
    unsigned long long m = 0;
    for (; i < nseg; i += stride) {
        unsigned long long l = ptr[i + 1] - ptr[i];
        m = l > m ? l : m;
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        unsigned long long o = __shfl_xor(m, d, 64);
        m = o > m ? o : m;
    }
    if ((threadIdx.x & 63) == 0) atomicMax(out, m);
}

// largest position (low word) among the column entries
__global__ void k_max_low32(const uint64_t *v, int64_t n, unsigned long long *out)
{
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    unsigned long long m = 0;
    for (; i < n; i += stride) { const unsigned long long l = (uint32_t)v[i]; m = l > m ? l : m; }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) { const unsigned long long o = __shfl_xor(m, d, 64); m = o > m ? o : m; }
    if ((threadIdx.x & 63) == 0) atomicMax(out, m);
}

// padded column store: slot j of column kid (at kid * stride + j) holds the column's j-th entry, or all ones behind its end; one lane per
// slot, so the stores of a wavefront are one contiguous 512 bytes (no fill pass before, no column-id array)
// The dense path's column store (a_ellj): the partner READS of column kid, right-aligned in the aligned block of Sj = 1 << jsh four-byte slots
// from kid * Sj — its L entries are the block's last L slots, all ones in front of them.  What a row entry owns (the column behind its own
// place) is then the tail of the block: one aligned 128-byte segment for every entry but the first ones of columns longer than 33.  Copied
// from the padded 8-byte store (whatever rotation it carries, k_fill_ell), one lane per 16-byte piece of the output.
// (ell == null: no rotation — the whole matrix —: the columns themselves, csc, are read instead of the padded store — 8 bytes per entry, not per slot)
__global__ void k_ell_partners(const uint64_t *ell, const uint64_t *csc, const uint32_t *colptr, uint64_t N, uint32_t S, uint32_t jsh, uint32_t *ellj, const uint32_t *label)
{
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x, nq = N << (jsh - 2u);
    const uint32_t Sj = 1u << jsh;
    for (uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; t < nq; t += stride) {
        const uint64_t kid = t >> (jsh - 2u);
        const uint32_t c0 = colptr[kid], s0 = ((uint32_t)t & ((Sj >> 2) - 1u)) << 2, L = colptr[kid + 1] - c0;
        const uint64_t *col = ell ? ell + kid * S : csc + c0;
        uint4 v;
        v.x = s0 + L >= Sj ? (uint32_t)(col[s0 + L - Sj] >> 32) : 0xFFFFFFFFu;
        v.y = s0 + 1u + L >= Sj ? (uint32_t)(col[s0 + 1u + L - Sj] >> 32) : 0xFFFFFFFFu;
        v.z = s0 + 2u + L >= Sj ? (uint32_t)(col[s0 + 2u + L - Sj] >> 32) : 0xFFFFFFFFu;
        v.w = s0 + 3u + L >= Sj ? (uint32_t)(col[s0 + 3u + L - Sj] >> 32) : 0xFFFFFFFFu;
        if (label) {      // (partners by their LABEL — Ctx::row_label: reads of one locus get neighbouring labels)
            if (v.x != 0xFFFFFFFFu) v.x = label[v.x];
            if (v.y != 0xFFFFFFFFu) v.y = label[v.y];
            if (v.z != 0xFFFFFFFFu) v.z = label[v.z];
            if (v.w != 0xFFFFFFFFu) v.w = label[v.w];
        }
        reinterpret_cast<uint4 *>(ellj)[t] = v;
    }
}
// colw0 (dense matrices with a row window): column kid is stored ROTATED by colw0[kid] = its entries of reads below the window — the window's
// entries first, then the reads above it, then the reads below it.  With pairs owned by the smaller row INSIDE the window and every partner
// outside it kept (owns_pair), the candidates a window row's entry owns are then exactly the slots behind its own, as without a window.
// (Relative order inside each of the three groups is kept, so a product's sequence number still orders the products of one pair.)
__global__ void k_col_w0(const uint32_t *colptr, const uint64_t *csc, uint64_t N, uint32_t win_lo, uint8_t *colw0)
{
    const uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= N) return;
    const uint32_t c0 = colptr[k], L = colptr[k + 1] - c0;
    uint32_t w0 = 0;
    while (w0 < L && (uint32_t)(csc[c0 + w0] >> 32) < win_lo) ++w0;
    colw0[k] = (uint8_t)(w0 == L ? 0u : w0);      // (a column wholly below the window — it holds no window row — keeps its order)
}
__global__ void k_fill_ell(const uint32_t *colptr, const uint64_t *csc, uint64_t nslots, uint32_t cs, uint64_t *ell, const uint8_t *colw0)
{
    // two slots (16 bytes) per lane: the stride is even, so a pair never straddles two columns.  (Adding the hint bits of the entries here, by the lane
    // that copies them, was measured: 15.8 ms against 4.8 + 5.2 for this kernel and k_add_hints — most lanes hold padding.)
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x, npairs = nslots >> 1;
    for (uint64_t t2 = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; t2 < npairs; t2 += stride) {
        const uint64_t t = t2 << 1, kid = t / cs;
        const uint32_t j = (uint32_t)(t - kid * cs), c0 = colptr[kid], L = colptr[kid + 1] - c0, w0 = colw0 ? colw0[kid] : 0u;
        ulonglong2 v;
        v.x = j < L ? csc[c0 + (j + w0 < L ? j + w0 : j + w0 - L)] : ~0ull;
        v.y = j + 1u < L ? csc[c0 + (j + 1u + w0 < L ? j + 1u + w0 : j + 1u + w0 - L)] : ~0ull;
        reinterpret_cast<ulonglong2 *>(ell)[t2] = v;
    }
}

// dense matrices: smallest k-mer id of the row << 32 | row (an empty row: behind all others); the sorted keys give label -> row and row -> label
__global__ void k_row_minimizer(const uint32_t *rowptr, const uint64_t *csr, uint32_t M, uint64_t N, uint64_t *keys)
{
    const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= M) return;
    const uint32_t rs = rowptr[r], re = rowptr[r + 1];
    const uint64_t kid = rs < re ? csr[rs] >> 32 : N;      // (dense row entries: k-mer id in the upper word)
    keys[r] = kid << 32 | r;
}
__global__ void k_order_and_labels(const uint64_t *keys, uint32_t M, uint32_t *order, uint32_t *label)
{
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t < M) { const uint32_t r = (uint32_t)keys[t]; order[t] = r; label[r] = t; }
}

}  // namespace

int64_t max_segment_len(Ctx &c, const uint32_t *ptr, int64_t nseg)
{
    if (nseg <= 0) return 0;
    c.ws_scan.reserve(64);
    ELBA_HIP(hipMemsetAsync(c.ws_scan.p, 0, 8, c.stream));
    int64_t nb = (nseg + 255) / 256;
    if (nb > 2048) nb = 2048;
    hipLaunchKernelGGL(k_max_seg_len, dim3((unsigned)nb), dim3(256), 0, c.stream, ptr, nseg, c.ws_scan.as<unsigned long long>());
    uint64_t h = 0;
    ELBA_HIP(hipMemcpyAsync(&h, c.ws_scan.p, 8, hipMemcpyDeviceToHost, c.stream));
    ELBA_HIP(hipStreamSynchronize(c.stream));
    return (int64_t)h;
}

// The column store the SpGEMM gathers from: padded columns (no column longer than 64 entries — UPPER <= 64: every configuration the reference
// documents — and room for the padding), column kid at kid * S, its address arithmetic, read by a group of S/2 lanes as one aligned segment; else the
// plain CSC, reached through a_colptr (csr_plan.hpp: plan_column_store decides).
// Sets use_ell, s_stride, lpc_log2, fbits and reserves a_ell (guard words written); the caller fills it.
void choose_column_store(Ctx &c, int64_t N, int64_t max_col)
{
    size_t free_b = 0, total_b = 0;
    ELBA_HIP(hipMemGetInfo(&free_b, &total_b));
    const ColumnStore st = plan_column_store(N, max_col, c.opt.no_ell, free_b + c.a_ell.cap);
    if (!st.padded && st.wanted && c.opt.trace)
        fprintf(stderr, "[elba] the padded column store (%zu bytes) does not fit a third of the free device memory (%zu bytes): columns are gathered from CSC\n", st.bytes, free_b + c.a_ell.cap);
    c.use_ell = st.padded; c.s_stride = st.stride; c.lpc_log2 = st.lpc_log2; c.fbits = st.fbits;
    c.ell_compact = false; c.ell_nslots = c.use_ell ? N : 0; c.ell_cap_cols = c.use_ell ? N : 0;      // (kmer_msd.hip may compact the store: gather slots)
    if (c.use_ell) {
        c.a_ell.reserve(st.bytes + 64);
        ELBA_HIP(hipMemsetAsync(c.a_ell.as<char>() + st.bytes, 0xFF, 64, c.stream));      // (guard words behind the last column)
    }
}

namespace {

// ---- finish_matrix_from_sorted_csc: what its steps share, and the steps -------------------------------------------------------------------
struct CsrBuild {
    Ctx &c;
    const int64_t M, N, Z;
    const uint64_t *kid_keys; int kid_shift;
    const bool pre;                 // the k-mer stage left the column pointers, a bound on the positions and the CSR sort's input behind (Ctx::pre)
    hipStream_t s = c.stream;
    bool windowed = false; uint32_t wlo = 0, whi = 0;
    uint64_t maxpos = 0;
    const uint8_t *colw0 = nullptr;
    CsrBuildPlan p;
    const uint32_t *colptr() const { return c.a_colptr.as<uint32_t>(); }
    const uint64_t *columns() const { return c.a_csc.as<uint64_t>(); }
    unsigned long long *prod_ctr() const { return c.prod_ctr.as<unsigned long long>(); }
    DevBuf &ws(CsrBuf b) const { return b == CSR_WS_A ? c.ws_a : b == CSR_WS_B ? c.ws_b : b == CSR_WS_C ? c.ws_c : c.ws_d; }
    static unsigned blocks(int64_t n) { return (unsigned)((n + 255) / 256); }

    // the matrix's size, its buffers, the columns in a_csc, the largest position among the entries: below 2^16 the SpGEMM's 64-bit accumulators carry both
    // positions of a seed (spgemm_direct.hpp); it also decides whether an entry fits one word for the CSR sort
    void size_and_maxpos(const uint64_t *csc, int64_t win_lo, int64_t win_hi)
    {
        c.M = M; c.N = N; c.Z = Z;
        c.a_colptr.reserve((size_t)(N + 1) * 4);
        c.a_rowptr.reserve((size_t)(M + 1) * 4);
        c.a_csc.reserve((size_t)(Z + 8) * 8);   // + guard entries: the SpGEMM gathers up to four consecutive entries without a bounds check
        c.a_csr.reserve((size_t)(Z + 1) * 8);
        if (!pre) group_offsets_u32(s, kid_keys, kid_shift, Z, c.a_colptr.as<uint32_t>(), N);
        if (csc != columns() && Z > 0) ELBA_HIP(hipMemcpyAsync(c.a_csc.p, csc, (size_t)Z * 8, hipMemcpyDeviceToDevice, s));
        maxpos = pre ? c.pre.maxpos : 0;
        if (Z > 0 && !pre) {
            c.ws_scan.reserve(64);
            ELBA_HIP(hipMemsetAsync(c.ws_scan.p, 0, 8, s));
            hipLaunchKernelGGL(k_max_low32, dim3(std::min(blocks(Z), 2048u)), dim3(256), 0, s, columns(), Z, c.ws_scan.as<unsigned long long>());
            ELBA_HIP(hipMemcpyAsync(&maxpos, c.ws_scan.p, 8, hipMemcpyDeviceToHost, s));
            ELBA_HIP(hipStreamSynchronize(s));
        }
        ELBA_REQUIRE(win_lo >= 0 && (win_hi < 0 || (win_lo <= win_hi && win_hi <= M)), ELBA_ERR_INVALID_ARG, "bad row window");
        windowed = !(win_lo == 0 && (win_hi < 0 || win_hi == M));
        wlo = (uint32_t)win_lo; whi = (uint32_t)(win_hi < 0 ? M : win_hi);
        c.ws_a.reserve((size_t)(Z + 1) * 8); c.ws_c.reserve((size_t)(Z + 1) * 8);      // (the CSR sort's buffers)
        c.prod_ctr.reserve(64 * 128);
        if (!pre) ELBA_HIP(hipMemsetAsync(prod_ctr(), 0, 64 * 128, s));      // (pre: the producer has counted)
    }
    // the column store, unless the producer chose and filled it (the two-level partition of kmer_msd.hip writes the padded columns with the columns themselves)
    void column_store()
    {
        if (pre && c.pre.ell_done) return;
        c.max_col_nnz = max_segment_len(c, colptr(), N);
        choose_column_store(c, N, c.max_col_nnz);
    }
    void plan()
    {
        CsrBuildInput in;
        in.M = M; in.N = N; in.Z = Z; in.maxpos = maxpos; in.windowed = windowed; in.use_ell = c.use_ell; in.ell_compact = c.ell_compact; in.max_col = c.max_col_nnz;
        in.pre = pre ? &c.pre : nullptr; in.opt = csr_options(c);
        p = plan_csr_build(in);
    }
    // A dense matrix with a row window (a shard, a row block of a shard: elba_dist_set_panel): the padded columns are stored rotated (k_col_w0) so that a
    // row entry's owned candidates stay the column's entries behind its own.  Then the padded columns themselves.
    void fill_columns()
    {
        if (p.suffix && windowed && N > 0) {
            c.col_w0.reserve((size_t)N + 16);
            hipLaunchKernelGGL(k_col_w0, dim3(blocks(N)), dim3(256), 0, s, colptr(), columns(), (uint64_t)N, wlo, c.col_w0.as<uint8_t>());
            colw0 = c.col_w0.as<uint8_t>();
        }
        if (!(pre && c.pre.ell_done) && c.use_ell) {
            const uint64_t nslots = (uint64_t)N * c.s_stride;
            hipLaunchKernelGGL(k_fill_ell, dim3((unsigned)std::min<uint64_t>((nslots / 2 + 255) / 256, 1ull << 30)), dim3(256), 0, s, colptr(), columns(), nslots, c.s_stride, c.a_ell.as<uint64_t>(), colw0);
        }
    }
    void require_match() const
    {
        ELBA_REQUIRE(p.mismatch != CSR_WORDS_DO_NOT_MATCH, ELBA_ERR_INTERNAL, "create_kmer_matrix: the sort keys of the k-mer stage do not match the matrix");
        ELBA_REQUIRE(p.mismatch != CSR_PAIRS_NOT_DENSE, ELBA_ERR_INTERNAL, "create_kmer_matrix: the k-mer stage wrote the pairs of a dense matrix, the matrix is not one");
    }
    // ONE word per entry, sorted on the read bits (stable: rows come out ordered by (kid, pos)).  The keys are the hand-off's (hint bits and inline
    // partners added where it left them out) or written here.
    void build_one_word()
    {
        uint64_t *w0 = p.have_words ? c.csr_words.as<uint64_t>() : c.ws_a.as<uint64_t>(), *w1 = c.ws_c.as<uint64_t>();
        if (p.write_words)
            hipLaunchKernelGGL(k_csc_to_csr_words, dim3(blocks(Z)), dim3(256), 0, s, kid_keys, kid_shift, colptr(), columns(), Z, p.nb, p.pb, p.rs, p.write_pbi, w0, p.hints, wlo, whi, prod_ctr());
        if (p.add_hints) hipLaunchKernelGGL(k_add_hints, dim3(blocks(Z)), dim3(256), 0, s, colptr(), columns(), Z, p.nb, p.pb, p.rs, p.add_pbi, w0);
        if (p.fin_sort) {
            // the sort's last pass writes the rows themselves and their pointers (prims.hip: k_rs_scatter<FIN>): no pass over the sorted keys behind it
            // (round 4: k_unpack_csr_words read and wrote all of them once more — 1.9 ms of the 10 ms CSR build of BASELINE config 3)
            radix_sort_keys_to_csr(s, w0, w1, Z, CsrFin{p.idbits, p.pb, p.rs, p.mb, p.pbi_used, c.a_csr.as<uint64_t>(), c.a_rowptr.as<uint32_t>(), M}, c.ws_sort);
        } else {
            const int where = radix_sort_keys(s, w0, w1, Z, p.rs, p.rs + p.mb, c.ws_sort);
            hipLaunchKernelGGL(k_unpack_csr_words, dim3(blocks(Z + 1)), dim3(256), 0, s, (const uint64_t *)(where ? w1 : w0), Z, p.idbits, p.pb, p.rs, p.mb, p.pbi_used, c.a_csr.as<uint64_t>(), c.a_rowptr.as<uint32_t>(), M);
        }
    }
    // (read, entry) pairs, row ids as 32-bit keys (12 bytes per pair and pass).  The sorted values are the rows of A: the sort's buffers are handed over so
    // that it ENDS in a_csr (no copy behind it).  The pairs are the hand-off's (a dense matrix from kmer_msd.hip) or written here.
    void build_pairs()
    {
        c.ws_b.reserve((size_t)(Z + 1) * 8); c.ws_d.reserve((size_t)(Z + 1) * 8);
        const bool ends_in_second = radix_sort_where(Z, 0, p.mb) != 0;
        uint32_t *k0 = ws(p.k0).as<uint32_t>(), *k1 = ws(p.k1).as<uint32_t>();
        uint64_t *spare = ws(p.spare).as<uint64_t>(), *v0 = ends_in_second ? spare : c.a_csr.as<uint64_t>(), *v1 = ends_in_second ? c.a_csr.as<uint64_t>() : spare;
        if (p.rewrite_pairs) {
            const uint64_t *kk = p.key_source == CSR_KEYS_VALUES ? v0 : p.key_source == CSR_KEYS_WORDS ? c.csr_words.as<uint64_t>() : kid_keys;
            if (p.recount) ELBA_HIP(hipMemsetAsync(prod_ctr(), 0, 64 * 128, s));
            hipLaunchKernelGGL(k_csc_to_csr_keys, dim3(blocks(Z)), dim3(256), 0, s, kk, p.key_source == CSR_KEYS_CALLER ? kid_shift : p.key_shift, p.key_mask, colptr(), columns(), Z, k0, v0,
                               p.hints, p.suffix, wlo, whi, prod_ctr(), colw0);
        }
        const int where = radix_sort_pairs_k32(s, k0, v0, k1, v1, Z, 0, p.mb, c.ws_sort);
        ELBA_REQUIRE((where != 0) == ends_in_second, ELBA_ERR_INTERNAL, "create_kmer_matrix: the CSR sort ended in the other buffer");
        group_offsets_k32(s, where ? k1 : k0, Z, c.a_rowptr.as<uint32_t>(), M);
    }
    // the window's products (what the SpGEMM reports), counted on 64 counters by the kernel that saw every entry's column
    void read_product_count()
    {
        unsigned long long hp[64 * 16];
        ELBA_HIP(hipMemcpyAsync(hp, prod_ctr(), sizeof(hp), hipMemcpyDeviceToHost, s));
        ELBA_HIP(hipStreamSynchronize(s));
        c.A_products = 0;
        for (int q = 0; q < 64; ++q) c.A_products += (int64_t)hp[q * 16];
    }
    // A new matrix: the tier queues and the tier / sort usage of the previous one are forgotten.  The OUTPUT capacity is kept as a guess (the buffers
    // exist): the first SpGEMM call on this matrix then runs without a host round trip in its middle and checks afterwards that everything fitted
    // (spgemm.hip repeats the call on the synchronising path otherwise)
    void forget_previous_matrix()
    {
        c.ov_tiers_known = false; c.ov_sort_used[0] = c.ov_sort_used[1] = true;
        c.ov_prior_q16 = 0;            // forget the partner/product ratio measured on the previous one
        c.ov_slab_q16 = 0;
        c.ov_phase = 0;                // ... and a sharded call that was begun on the previous one
    }
    void longest_row()
    {
        c.max_row_nnz = max_segment_len(c, c.a_rowptr.as<uint32_t>(), M);
        ELBA_REQUIRE(c.fbits < 31 && (uint64_t)c.max_row_nnz < (1ull << (32 - c.fbits)), ELBA_ERR_UNSUPPORTED, "row nnz x column nnz exceeds the 32-bit product sequence number");
    }
    // Dense matrices: a row meets the same ~100 partners tens of thousands of times, and what its accumulator pays for is every look-up that
    // does not find its partner in the slot its hash names (it queues for the general insert: profiles/r03_notes.md).  Partner ids are random
    // — reads that overlap stand anywhere in the input — so the keys of a table collide as random keys do.  Reads of one locus share their
    // MINIMIZER, the smallest k-mer id of the row (its first entry: rows are in column order): ~20 reads of a 40x set share one.  The rows
    // sorted by minimizer give every read a LABEL (its rank); a row's partners are then a handful of runs of consecutive labels, which the
    // multiplicative hash keeps apart (config 5 / 25: 10.1 -> 9.7 ms).  The partner store of the dense path (a_ellj) holds labels, the
    // table is keyed by them, and the kernel turns the few surviving partners back into rows when it writes them.
    void row_order_and_partners()
    {
        if (p.row_order) {
            c.row_order.reserve((size_t)M * 4 + 64); c.row_label.reserve((size_t)M * 4 + 64);
            c.row_keys.reserve((size_t)(M + 1) * 16);
            uint64_t *k0 = c.row_keys.as<uint64_t>(), *k1 = k0 + (M + 1);
            hipLaunchKernelGGL(k_row_minimizer, dim3(blocks(M)), dim3(256), 0, s, (const uint32_t *)c.a_rowptr.as<uint32_t>(), (const uint64_t *)c.a_csr.as<uint64_t>(), (uint32_t)M, (uint64_t)N, k0);
            const int where = radix_sort_keys(s, k0, k1, M, 32, 32 + bits_needed((uint64_t)(N > 0 ? N : 1)), c.ws_sort);
            hipLaunchKernelGGL(k_order_and_labels, dim3(blocks(M)), dim3(256), 0, s, (const uint64_t *)(where ? k1 : k0), (uint32_t)M, c.row_order.as<uint32_t>(), c.row_label.as<uint32_t>());
        }
        if (p.suffix) {
            const uint64_t nslots = (uint64_t)N << p.j_shift;
            c.a_ellj.reserve((size_t)nslots * 4 + 64);
            hipLaunchKernelGGL(k_ell_partners, dim3((unsigned)std::min<uint64_t>((nslots / 4 + 255) / 256, 1ull << 20)), dim3(256), 0, s, windowed ? (const uint64_t *)c.a_ell.as<uint64_t>() : (const uint64_t *)nullptr, columns(), colptr(), (uint64_t)N, c.s_stride,
                               p.j_shift, c.a_ellj.as<uint32_t>(), p.row_order ? (const uint32_t *)c.row_label.as<uint32_t>() : (const uint32_t *)nullptr);
        }
    }
    // the format of the resident A, for everything that reads it
    void publish_format(int64_t win_lo, int64_t win_hi)
    {
        c.pos16 = p.pos16; c.csr_hints = p.hints; c.csr_suffix = p.suffix; c.csr_one_word = p.one_word;
        c.csr_inline = p.inl != CSR_INL_NONE; c.csr_inline_window = p.inline_window;
        if (p.suffix) c.j_shift = p.j_shift;
        c.have_row_order = p.row_order;
        c.row_lo = win_lo; c.row_hi = win_hi;
    }
};

}  // namespace

// Input: Z entries sorted by (kid, read, pos): kid_keys[z] >> kid_shift = kid, csc[z] = read<<32|pos (device, in c.a_csc or elsewhere).
// Produces c.a_colptr, c.a_csc (copy if csc is not already c.a_csc), c.a_rowptr, c.a_csr, max_row_nnz, max_col_nnz.
// [win_lo, win_hi) = the rows of B this context computes (win_hi < 0: all); the product schedule is laid out for those rows only.
// pre: the hand-off of the k-mer stage (Ctx::pre) is this matrix's.  Every decision is plan_csr_build's (csr_plan.hpp); the steps launch what it says.
void finish_matrix_from_sorted_csc(Ctx &c, int64_t M, int64_t N, int64_t Z, const uint64_t *kid_keys, int kid_shift, const uint64_t *csc, int64_t win_lo, int64_t win_hi, bool pre)
{
    CsrBuild b{c, M, N, Z, kid_keys, kid_shift, pre};
    b.size_and_maxpos(csc, win_lo, win_hi);
    b.column_store();
    b.plan();
    b.fill_columns();
    b.require_match();
    if (b.p.one_word) b.build_one_word(); else b.build_pairs();
    b.read_product_count();
    b.forget_previous_matrix();
    b.longest_row();
    b.row_order_and_partners();
    b.publish_format(win_lo, win_hi);
}

namespace {
// device triples -> (key = pos, value = col << 32 | row) pairs of the three-pass sort; out-of-range indices are counted, the largest position kept
__global__ void k_pack_triples(const int64_t *rows, const int64_t *cols, const uint32_t *vals, int64_t Z, int64_t M, int64_t N, uint64_t *k0, uint64_t *v0, unsigned long long *chk)
{
    const int64_t z = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    unsigned long long bad = 0, mx = 0;
    if (z < Z) {
        const int64_t r = rows[z], cc = cols[z];
        const uint32_t v = vals[z];
        if (r < 0 || r >= M || cc < 0 || cc >= N) bad = 1;
        else { k0[z] = v; v0[z] = ((uint64_t)cc << 32) | (uint64_t)r; mx = v; }
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) { bad += __shfl_xor(bad, d, 64); const unsigned long long o = __shfl_xor(mx, d, 64); mx = o > mx ? o : mx; }
    // (one hot word: a wavefront only touches it when it would raise it — 8 M wavefronts each doing an atomic on it took 95 ms)
    if ((threadIdx.x & 63) == 0) { if (bad) atomicAdd(&chk[0], bad); if (mx > __hip_atomic_load(&chk[1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(&chk[1], mx); }
}
// the same check alone (out-of-range indices counted, largest position kept): what the one-word sort needs to know before it packs
__global__ void k_check_triples(const int64_t *rows, const int64_t *cols, const uint32_t *vals, int64_t Z, int64_t M, int64_t N, unsigned long long *chk)
{
    const int64_t z = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    unsigned long long bad = 0, mx = 0;
    if (z < Z) {
        const int64_t r = rows[z], cc = cols[z];
        if (r < 0 || r >= M || cc < 0 || cc >= N) bad = 1; else mx = vals[z];
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) { bad += __shfl_xor(bad, d, 64); const unsigned long long o = __shfl_xor(mx, d, 64); mx = o > mx ? o : mx; }
    if ((threadIdx.x & 63) == 0) { if (bad) atomicAdd(&chk[0], bad); if (mx > __hip_atomic_load(&chk[1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(&chk[1], mx); }
}
// device triples -> ONE sort word each, col << (mb + pb) | row << pb | pos: sorted as 64-bit keys they are in (col, row, pos) order
__global__ void k_pack_triple_words(const int64_t *rows, const int64_t *cols, const uint32_t *vals, int64_t Z, int mb, int pb, uint64_t *w)
{
    const int64_t z = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (z < Z) w[z] = ((uint64_t)cols[z] << (mb + pb)) | ((uint64_t)rows[z] << pb) | (uint64_t)vals[z];
}
// sorted words -> what finish_matrix_from_sorted_csc takes: col << 32 | row and row << 32 | pos
__global__ void k_unpack_triple_words(const uint64_t *w, int64_t Z, int mb, int pb, uint64_t *keys, uint64_t *csc)
{
    const int64_t z = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (z >= Z) return;
    const uint64_t x = w[z], row = (x >> pb) & ((1ull << mb) - 1), pos = x & ((1ull << pb) - 1);
    keys[z] = ((x >> (mb + pb)) << 32) | row;
    csc[z] = (row << 32) | pos;
}
// A as triples, from the resident matrix (rows: the context's row ids, cols: k-mer ids, vals: positions), in CSR order
__global__ void k_export_triples(const uint32_t *rowptr, const uint64_t *csr, uint32_t M, uint32_t pos_mask, int64_t *rows, int64_t *cols, uint32_t *vals)
{
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6, nwaves = (gridDim.x * blockDim.x) >> 6;
    for (uint32_t i = wave; i < M; i += nwaves)
        for (uint32_t e = rowptr[i] + lane, re = rowptr[i + 1]; e < re; e += 64) { const uint64_t x = csr[e]; rows[e] = i; cols[e] = (int64_t)(x >> 32); vals[e] = (uint32_t)x & pos_mask; }
}
__global__ void k_export_triples_csc(const uint32_t *colptr, const uint64_t *csc, uint64_t N, int64_t *rows, int64_t *cols, uint32_t *vals)
{
    const uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= N) return;
    for (uint32_t z = colptr[k], z1 = colptr[k + 1]; z < z1; ++z) { rows[z] = (int64_t)(csc[z] >> 32); cols[z] = (int64_t)k; vals[z] = (uint32_t)csc[z]; }
}
}  // namespace

// k0 / v0 (= c.ws_a / c.ws_b) hold (pos, col << 32 | row) of every triple
static void set_kmer_matrix_from_pairs(Ctx &c, int64_t M, int64_t N, int64_t Z, uint64_t maxpos)
{
    hipStream_t s = c.stream;
    uint64_t *k0 = c.ws_a.as<uint64_t>(), *v0 = c.ws_b.as<uint64_t>(), *k1 = c.ws_c.as<uint64_t>(), *v1 = c.ws_d.as<uint64_t>();
    // (1) by pos, (2) by row, (3) by col — LSD, stable: final order (col, row, pos)
    int w = radix_sort_pairs(s, k0, v0, k1, v1, Z, 0, bits_needed(maxpos), c.ws_sort);
    // swap roles: key := (col<<32|row), value := pos
    uint64_t *ck = w ? v1 : v0, *cv = w ? k1 : k0, *ok = w ? v0 : v1, *ov = w ? k0 : k1;
    int w2 = radix_sort_pairs(s, ck, cv, ok, ov, Z, 0, bits_needed((uint64_t)(M > 0 ? M - 1 : 0)), c.ws_sort);
    if (w2) { uint64_t *t; t = ck; ck = ok; ok = t; t = cv; cv = ov; ov = t; }
    int w3 = radix_sort_pairs(s, ck, cv, ok, ov, Z, 32, 32 + bits_needed((uint64_t)(N > 0 ? N - 1 : 0)), c.ws_sort);
    if (w3) { uint64_t *t; t = ck; ck = ok; ok = t; t = cv; cv = ov; ov = t; }
    // ck = (col<<32|row) sorted, cv = pos.  Move the keys out of the ws_a..d pool (finish_* reuses it).
    uint64_t *keys = c.ws_e.as<uint64_t>();
    uint64_t *csc = c.ws_f.as<uint64_t>();
    if (Z > 0) {
        ELBA_HIP(hipMemcpyAsync(keys, ck, (size_t)Z * 8, hipMemcpyDeviceToDevice, s));
        int64_t nb = (Z + 255) / 256;
        hipLaunchKernelGGL(k_colrow_to_csc, dim3((unsigned)nb), dim3(256), 0, s, ck, cv, Z, csc);
    }
    c.A_has_kmers = false;
    finish_matrix_from_sorted_csc(c, M, N, Z, keys, 32, csc);
}

void stage_set_kmer_matrix_device(Ctx &c, int64_t M, int64_t N, int64_t Z, const int64_t *d_rows, const int64_t *d_cols, const uint32_t *d_vals)
{
    enter(c.v, EV_SET_KMER_MATRIX_DEVICE);
    ELBA_REQUIRE(M >= 0 && N >= 0 && Z >= 0, ELBA_ERR_INVALID_ARG, "negative matrix dimension");
    ELBA_REQUIRE(M < 0xFFFFFFFFll && N < 0xFFFFFFFFll && Z < 0xFFFFFFFFll, ELBA_ERR_UNSUPPORTED, "matrix dimension beyond 32-bit device indices");
    ELBA_REQUIRE(Z == 0 || (d_rows && d_cols && d_vals), ELBA_ERR_INVALID_ARG, "null triple array");
    accepted(c.v, EV_SET_KMER_MATRIX_DEVICE);       // (before the device checks the indices: the bucket kernels write into A's buffers as they check)
    hipStream_t s = c.stream;
    c.ws_scan.reserve(64);
    const unsigned nbz = (unsigned)((Z + 255) / 256);
    // Matrices of some size whose columns all hold entries (the reference's A: a reliable k-mer occurs LOWER times at least) go through the k-mer stage's
    // bucket kernels — two-level partition by column, every bucket of ~256 columns sorted in LDS, columns, hints, inline partners, gather slots and the
    // CSR build's sort keys written from there (kmer_msd.hip; it checks the indices as it packs them) — instead of seven radix passes over the whole
    // matrix and a pass per by-product
    c.triples_path = 0;
    if (msd_matrix_from_triples(c, M, N, Z, d_rows, d_cols, d_vals)) {
        c.triples_path = 1;
        c.A_has_kmers = false;
        finish_matrix_from_sorted_csc(c, M, N, Z, nullptr, 0, c.a_csc.as<uint64_t>(), 0, -1, true);
        c.pre.consume();
        done(c.v, EV_SET_KMER_MATRIX_DEVICE);
        return;
    }
    ELBA_HIP(hipMemsetAsync(c.ws_scan.p, 0, 16, s));
    if (Z > 0) hipLaunchKernelGGL(k_check_triples, dim3(nbz), dim3(256), 0, s, d_rows, d_cols, d_vals, Z, M, N, c.ws_scan.as<unsigned long long>());
    unsigned long long chk[2] = {0, 0};
    ELBA_HIP(hipMemcpyAsync(chk, c.ws_scan.p, 16, hipMemcpyDeviceToHost, s));
    ELBA_HIP(hipStreamSynchronize(s));
    ELBA_REQUIRE(chk[0] == 0, ELBA_ERR_INVALID_ARG, "triple index out of range");
    c.ws_a.reserve((size_t)(Z + 1) * 8); c.ws_b.reserve((size_t)(Z + 1) * 8);
    c.ws_c.reserve((size_t)(Z + 1) * 8); c.ws_d.reserve((size_t)(Z + 1) * 8);
    c.ws_e.reserve((size_t)(Z + 1) * 8); c.ws_f.reserve((size_t)(Z + 1) * 8);
    // k-mer id, read and position in ONE 64-bit word when they fit (28 + 18 + 14 bits on the 200 k-read set): one sort of 8-byte keys over
    // all their bits instead of three stable sorts of 16-byte (key, value) pairs — 7 passes of ~3 ms instead of 8 of ~7 ms there
    const int mb = bits_needed((uint64_t)(M > 0 ? M - 1 : 0)), nb = bits_needed((uint64_t)(N > 0 ? N - 1 : 0)), pb = bits_needed(chk[1]);
    if (mb + nb + pb <= 64 && Z > 0 && !c.opt.csr_pairs) {
        uint64_t *w0 = c.ws_a.as<uint64_t>(), *w1 = c.ws_b.as<uint64_t>();
        hipLaunchKernelGGL(k_pack_triple_words, dim3(nbz), dim3(256), 0, s, d_rows, d_cols, d_vals, Z, mb, pb, w0);
        const int where = radix_sort_keys(s, w0, w1, Z, 0, mb + nb + pb, c.ws_sort);
        hipLaunchKernelGGL(k_unpack_triple_words, dim3(nbz), dim3(256), 0, s, (const uint64_t *)(where ? w1 : w0), Z, mb, pb, c.ws_e.as<uint64_t>(), c.ws_f.as<uint64_t>());
        c.A_has_kmers = false;
        finish_matrix_from_sorted_csc(c, M, N, Z, c.ws_e.as<uint64_t>(), 32, c.ws_f.as<uint64_t>());
        done(c.v, EV_SET_KMER_MATRIX_DEVICE);
        return;
    }
    if (Z > 0)
        hipLaunchKernelGGL(k_pack_triples, dim3(nbz), dim3(256), 0, s, d_rows, d_cols, d_vals, Z, M, N, c.ws_a.as<uint64_t>(), c.ws_b.as<uint64_t>(), c.ws_scan.as<unsigned long long>());
    ELBA_HIP(hipStreamSynchronize(s));
    set_kmer_matrix_from_pairs(c, M, N, Z, chk[1]);
    done(c.v, EV_SET_KMER_MATRIX_DEVICE);
}

void stage_export_triples_device(Ctx &c, int64_t *d_rows, int64_t *d_cols, uint32_t *d_vals)
{
    ELBA_REQUIRE(has(c.v, P_A), ELBA_ERR_STATE, "export_triples_device: no k-mer matrix");
    ELBA_REQUIRE(c.Z == 0 || (d_rows && d_cols && d_vals), ELBA_ERR_INVALID_ARG, "null triple array");
    if (c.csr_inline && c.N > 0 && c.Z > 0) {      // (rows with inline partners do not name every entry's k-mer: the triples come from the columns)
        hipLaunchKernelGGL(k_export_triples_csc, dim3((unsigned)((c.N + 255) / 256)), dim3(256), 0, c.stream, (const uint32_t *)c.a_colptr.as<uint32_t>(), (const uint64_t *)c.a_csc.as<uint64_t>(), (uint64_t)c.N, d_rows, d_cols, d_vals);
    } else if (c.M > 0 && c.Z > 0) {
        int nb = (int)std::min<int64_t>((c.M + 3) / 4, (int64_t)c.num_cus * 32);
        hipLaunchKernelGGL(k_export_triples, dim3(nb), dim3(256), 0, c.stream, (const uint32_t *)c.a_rowptr.as<uint32_t>(), (const uint64_t *)c.a_csr.as<uint64_t>(), (uint32_t)c.M,
                           csr_pos_mask(c.csr_suffix, c.csr_hints), d_rows, d_cols, d_vals);
    }
    ELBA_HIP(hipStreamSynchronize(c.stream));
}

void stage_set_kmer_matrix(Ctx &c, int64_t M, int64_t N, int64_t Z, const int64_t *rows, const int64_t *cols, const uint32_t *vals)
{
    enter(c.v, EV_SET_KMER_MATRIX);
    ELBA_REQUIRE(M >= 0 && N >= 0 && Z >= 0, ELBA_ERR_INVALID_ARG, "negative matrix dimension");
    ELBA_REQUIRE(M < 0xFFFFFFFFll && N < 0xFFFFFFFFll && Z < 0xFFFFFFFFll, ELBA_ERR_UNSUPPORTED, "matrix dimension beyond 32-bit device indices");
    ELBA_REQUIRE(Z == 0 || (rows && cols && vals), ELBA_ERR_INVALID_ARG, "null triple array");
    hipStream_t s = c.stream;
    std::vector<uint64_t> hk((size_t)Z + 1), hv((size_t)Z + 1);
    uint32_t maxpos = 0;
    for (int64_t z = 0; z < Z; ++z) {
        ELBA_REQUIRE(rows[z] >= 0 && rows[z] < M && cols[z] >= 0 && cols[z] < N, ELBA_ERR_INVALID_ARG, "triple index out of range");
        hk[(size_t)z] = vals[z];
        hv[(size_t)z] = ((uint64_t)cols[z] << 32) | (uint64_t)rows[z];
        if (vals[z] > maxpos) maxpos = vals[z];
    }
    accepted(c.v, EV_SET_KMER_MATRIX);
    c.ws_a.reserve((size_t)(Z + 1) * 8); c.ws_b.reserve((size_t)(Z + 1) * 8);
    c.ws_c.reserve((size_t)(Z + 1) * 8); c.ws_d.reserve((size_t)(Z + 1) * 8);
    c.ws_e.reserve((size_t)(Z + 1) * 8); c.ws_f.reserve((size_t)(Z + 1) * 8);
    if (Z > 0) {
        ELBA_HIP(hipMemcpyAsync(c.ws_a.p, hk.data(), (size_t)Z * 8, hipMemcpyHostToDevice, s));
        ELBA_HIP(hipMemcpyAsync(c.ws_b.p, hv.data(), (size_t)Z * 8, hipMemcpyHostToDevice, s));
        ELBA_HIP(hipStreamSynchronize(s));      // (the host vectors go out of scope below)
    }
    set_kmer_matrix_from_pairs(c, M, N, Z, maxpos);
    done(c.v, EV_SET_KMER_MATRIX);
}

}  // namespace elba
