// csr_plan.hpp — the decisions of the CSR build of A (matrix.hip, finish_matrix_from_sorted_csc) and of the producers that prepare it (k_runs_emit's
// caller in kmer.hip, layout_output in kmer_msd.hip) as pure host arithmetic: the layout of a sort key (csr_key_layout), when a matrix is dense
// (csr_dense), the geometry of the column store (plan_column_store), what the k-mer stage hands to the build (CsrHandoff), everything the build
// decides (plan_csr_build) and the format of a row entry (csr_pos_mask, csr_format, csr_inline_word, csr_entry_of_word).  No HIP, no context: plain
// values in, plain values out — hostcpp/test_csr_plan.cpp walks them without a GPU.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>

// the row entry's helpers run in kernels too
#if defined(__HIPCC__)
#define ELBA_HD __host__ __device__
#else
#define ELBA_HD
#endif

namespace elba {

// bits of a field that holds values up to maxval (at least one)
inline int bits_needed(uint64_t maxval)
{
    int b = 1;
    while (b < 64 && (maxval >> b)) ++b;
    return b;
}
inline int bits_needed_u(uint64_t maxval) { return bits_needed(maxval); }      // (the name msd_plan.hpp's callers use)

// the options the build's decisions read (Ctx::opt's, by name; tune1: Ctx::opt.tune[1])
struct CsrOptions { bool csr_pairs = false, no_hints = false, no_pay = false, no_inline = false, no_symmetry = false, no_ell = false, no_suffix = false, panel_inline = false, no_row_order = false; long long tune1 = 0; };

// ---- the sort key --------------------------------------------------------------------------------------------------------------------------
// One word per entry when read, k-mer id, two hint bits and position fit 64 bits: read << rs | kid << (pb + 2) | hint << pb | pos, rs = nb + pb + 2.
// With inline partners (Ctx::csr_inline) the read sits as high as it goes below the flag, rs = 63 - mb, and an entry whose row accumulates exactly one
// pair of its column is flag | read << rs | (partner >> 1) << 2 pbi | posQ << pbi | posT: pbi position bits are what the word leaves, and they are
// only worth it from 10 bits on.
enum CsrInlineWhen { CSR_INLINE_NONE, CSR_INLINE_NOW, CSR_INLINE_PENDING };      // written by the producer itself | room left: k_add_hints writes them if the matrix qualifies
struct CsrKeyLayout { bool words = false, hints = false; int rs = 0, pbi = 0; CsrInlineWhen inl = CSR_INLINE_NONE; };
// what a producer knows of the matrix where it lays the key out: the padded column store is in use (or, before it is chosen, not ruled out), the
// matrix is known or guaranteed not to be dense, every position is below 2^16, the matrix has a row window
struct CsrProducer { bool padded = false, not_dense = false, pos16 = false, windowed = false; };
constexpr int CSR_INLINE_MIN_PBI = 10;
constexpr int64_t CSR_SPARSE_MAX_COL = 16;      // no column longer: the matrix cannot be dense (a producer that has not seen the columns asks UPPER)

inline CsrKeyLayout csr_key_layout(int mb, int nb, int pb, int64_t N, const CsrOptions &o, const CsrProducer &p, CsrInlineWhen when)
{
    CsrKeyLayout l;
    l.words = mb + nb + pb + 2 <= 64 && !o.csr_pairs;
    l.hints = pb <= 30 && !o.no_hints;
    l.rs = nb + pb + 2;
    // inline partners: the general (not dense) SpGEMM path with position-carrying accumulators on padded columns; the rule they follow is the parity
    // rule over ALL rows, so a windowed matrix gets them on request only ("panel_inline": it is then multiplied with the mirror exchange only)
    if (l.words && l.hints && p.padded && p.not_dense && p.pos16 && !o.no_pay && !o.no_inline && !o.no_symmetry && (!p.windowed || o.panel_inline) && N < (1ll << 31) && mb >= 2) {
        const int rs2 = 63 - mb, pbi = std::min(pb, (rs2 - (mb - 1)) / 2);
        if (rs2 >= l.rs && pbi >= CSR_INLINE_MIN_PBI) { l.rs = rs2; l.pbi = pbi; l.inl = when; }
    }
    return l;
}

// Dense matrices (columns of more than 16 reads, e.g. UPPER = 35 on 40x low-error reads): pairs are owned by their smaller row and a row entry carries its
// column's length and its own place in it (Ctx::csr_suffix).  Positions below 2^16, the padded column store.
inline bool csr_dense(bool use_ell, bool pos16, int64_t max_col, const CsrOptions &o) { return use_ell && pos16 && max_col > CSR_SPARSE_MAX_COL && !o.no_pay && !o.no_suffix; }

// ---- the column store ------------------------------------------------------------------------------------------------------------------------
// No column longer than 64 entries: columns padded to a common stride (4 entries, else the longest column rounded up to whole 64-byte lines — a
// power of two is not needed, the kernel multiplies), if that fits a third of the free device memory and 2^40 slots.  Otherwise the plain CSC.
// lpc_log2: lanes of the SpGEMM per row entry (padded: 16 bytes each; plain: half the longest column, between 2 and 64); fbits: bits of a product
// sequence number's place in the column.
struct ColumnStore { bool padded = false, wanted = false; uint32_t stride = 0, lpc_log2 = 1, fbits = 1; size_t bytes = 0; };
inline uint32_t column_stride(uint32_t max_col) { return max_col <= 4 ? 4u : (max_col + 7u) & ~7u; }
inline ColumnStore plan_column_store(int64_t N, int64_t max_col, bool no_ell, size_t free_bytes)
{
    ColumnStore s;
    const uint32_t mc = (uint32_t)(max_col > 0 ? max_col : 1), stride = column_stride(mc);
    s.bytes = (size_t)N * stride * 8;
    s.wanted = mc <= 64 && N > 0 && !no_ell;
    s.padded = s.wanted && s.bytes <= free_bytes / 3 && (uint64_t)N * stride < (1ull << 40);
    uint32_t lb = 1;
    if (s.padded) {
        uint32_t fb = 2;
        while ((2u << lb) < stride) ++lb;
        while ((1u << fb) < stride) ++fb;
        s.stride = stride; s.fbits = fb;
    } else {
        while (lb < 6 && (2u << lb) < mc) ++lb;
        int fb = 1;
        while (fb < 31 && ((uint64_t)(mc > 1 ? mc - 1 : 1) >> fb)) ++fb;
        s.fbits = (uint32_t)fb;
    }
    s.lpc_log2 = lb;
    return s;
}

// ---- the hand-off from elba_count_kmers (or the bucket kernels' triples path) to the build --------------------------------------------------
// A producer builds a complete value and assigns it once (Ctx::pre); the build that used it calls consume(): the sort keys / column ids are spent
// (hint bits ORed in, the sort ping-pongs over them) and a later build of the same counts rebuilds the column ids from the column pointers.
struct CsrHandoff {
    enum State { NONE, READY, CONSUMED } state = NONE;
    bool words = false;           // csr_words holds a sort key per entry of a_csc (layout: nb, pb, rs, pbi)
    bool hints = false;           // the matrix gets hint bits ...
    bool hints_done = false;      // ... and the keys carry them already
    bool ell_done = false;        // the column store is chosen and filled (kmer_msd.hip writes the padded columns with the columns themselves)
    bool inl = false;             // the keys carry inline partners
    bool inline_pending = false;  // the keys leave room for inline partners: k_add_hints writes them if the matrix qualifies
    bool pairs = false;           // dense matrix from kmer_msd.hip: the (read, kid | L | place | pos) pairs of the CSR sort are written (keys in ws_b; values where a
                                  // sort of Z pairs on the read bits that ENDS in a_csr starts: a_csr or ws_d)
    int nb = 0, pb = 0, rs = 0, pbi = 0;
    uint64_t maxpos = 0;          // a bound on the positions
    bool ready() const { return state == READY; }
    void consume() { *this = CsrHandoff{}; state = CONSUMED; }
};
inline CsrHandoff csr_handoff(const CsrKeyLayout &l, int nb, int pb, uint64_t maxpos)
{
    CsrHandoff h;
    h.state = CsrHandoff::READY; h.words = l.words; h.hints = l.hints; h.nb = nb; h.pb = pb; h.rs = l.rs; h.pbi = l.pbi; h.maxpos = maxpos;
    h.inl = l.inl == CSR_INLINE_NOW; h.inline_pending = l.inl == CSR_INLINE_PENDING;
    return h;
}

// ---- the build's plan --------------------------------------------------------------------------------------------------------------------------
enum CsrInlineFrom { CSR_INL_NONE, CSR_INL_WORDS, CSR_INL_HERE, CSR_INL_LATE };      // came with the hand-off's keys | k_csc_to_csr_words writes them | k_add_hints does
enum CsrMismatch { CSR_MATCH, CSR_WORDS_DO_NOT_MATCH, CSR_PAIRS_NOT_DENSE };
enum CsrKeySource { CSR_KEYS_CALLER, CSR_KEYS_WORDS, CSR_KEYS_VALUES };      // the k-mer id of entry z: the caller's keys | a field of the hand-off's sort word | the upper half of the pair's value
enum CsrBuf { CSR_WS_A, CSR_WS_B, CSR_WS_C, CSR_WS_D };
struct CsrBuildInput {
    int64_t M = 0, N = 0, Z = 0;
    uint64_t maxpos = 0;
    bool windowed = false;
    bool use_ell = false, ell_compact = false; int64_t max_col = 0;      // the column store chosen
    const CsrHandoff *pre = nullptr;      // null or not ready: none
    CsrOptions opt;
};
struct CsrBuildPlan {
    int mb = 0, nb = 0, pb = 0;
    bool pos16 = false, suffix = false, hints = false, one_word = false;
    uint32_t j_shift = 5; bool row_order = false;
    CsrMismatch mismatch = CSR_MATCH;
    // the one-word sort
    bool have_words = false, write_words = false, add_hints = false, fin_sort = false;      // keys from the hand-off | k_csc_to_csr_words | k_add_hints | the sort's last pass writes the rows
    int rs = 0, pbi = 0, idbits = 0, pbi_used = 0, write_pbi = 0, add_pbi = 0;
    CsrInlineFrom inl = CSR_INL_NONE; bool inline_window = false;
    // the pair sort
    bool pre_pairs = false, kid_in_words = false, rewrite_pairs = false, recount = false;
    CsrKeySource key_source = CSR_KEYS_CALLER; int key_shift = -1 /* the caller's */; uint64_t key_mask = ~0ull;
    CsrBuf k0 = CSR_WS_A, k1 = CSR_WS_C, spare = CSR_WS_B;
};

inline CsrBuildPlan plan_csr_build(const CsrBuildInput &in)
{
    CsrBuildPlan p;
    const CsrOptions &o = in.opt;
    const CsrHandoff none, &h = in.pre && in.pre->ready() ? *in.pre : none;
    const bool pre = h.ready();
    const int mb = p.mb = bits_needed((uint64_t)(in.M > 0 ? in.M - 1 : 0)), nb = p.nb = bits_needed((uint64_t)(in.N > 0 ? in.N - 1 : 0)), pb = p.pb = bits_needed(in.maxpos);
    p.pos16 = in.maxpos < 65536;
    p.suffix = csr_dense(in.use_ell, p.pos16, in.max_col, o);
    p.hints = !p.suffix && (pre ? h.hints : (pb <= 30 && !o.no_hints));
    if (p.suffix) p.j_shift = in.max_col <= 32 ? 5u : 6u;      // (use_ell: no column longer than 64)
    p.row_order = p.suffix && !o.no_row_order && in.M > 1 && in.Z > 0;
    p.one_word = !p.suffix && mb + nb + pb + 2 <= 64 && !o.csr_pairs;
    if (p.one_word) {
        p.have_words = pre && h.words && h.nb == nb && h.pb == pb;
        if (pre && !p.have_words) p.mismatch = CSR_WORDS_DO_NOT_MATCH;
        p.rs = p.have_words ? h.rs : nb + pb + 2; p.pbi = p.have_words ? h.pbi : 0;
        // a matrix that did not come from the k-mer stage of this context (triples, a panel of the sharded build): the keys, inline partners included, are written here
        if (!p.have_words && p.hints) {
            const CsrKeyLayout l = csr_key_layout(mb, nb, pb, in.N, o, CsrProducer{in.use_ell, true, p.pos16, in.windowed}, CSR_INLINE_NOW);
            if (l.inl == CSR_INLINE_NOW) { p.rs = l.rs; p.pbi = l.pbi; p.inl = CSR_INL_HERE; }
        }
        // (sort keys of the k-mer stage's sort path: they left room for inline partners — whether the matrix qualifies is known here)
        if (p.have_words && p.hints && !h.hints_done && h.inline_pending && in.use_ell && p.pos16 && !in.windowed) p.inl = CSR_INL_LATE;
        if (p.have_words && h.inl) p.inl = CSR_INL_WORDS;
        p.write_words = in.Z > 0 && !p.have_words; p.write_pbi = p.inl == CSR_INL_HERE ? p.pbi : 0;
        p.add_hints = in.Z > 0 && p.have_words && p.hints && !h.hints_done; p.add_pbi = p.inl == CSR_INL_LATE ? p.pbi : 0;
        // (gather slots, kmer_msd.hip: the id field of a key may hold a slot beyond the last k-mer id — slots are drawn in chunks — and is as wide as
        //  the key leaves room below the read)
        p.idbits = p.have_words && in.ell_compact ? std::min(32, p.rs - pb - 2) : nb;
        p.pbi_used = p.inl != CSR_INL_NONE ? p.pbi : 0;
        p.fin_sort = in.Z > 0 && in.M > 0 && o.tune1 != 1;
        p.inline_window = p.inl == CSR_INL_HERE && in.windowed;
    } else {
        p.pre_pairs = pre && h.pairs;
        if (pre && h.words && !p.suffix && !p.pre_pairs) p.mismatch = CSR_WORDS_DO_NOT_MATCH;
        else if (p.pre_pairs && !p.suffix) p.mismatch = CSR_PAIRS_NOT_DENSE;
        p.kid_in_words = pre && h.words && !p.pre_pairs;        // (k_runs_emit left sort keys, not column ids: the k-mer id is a field of the word)
        // (row ids as 32-bit keys.  Pairs that must be written again — a row window rotates the columns —: the k-mer id is the value's upper half)
        if (p.pre_pairs) { p.k0 = CSR_WS_B; p.k1 = CSR_WS_A; p.spare = CSR_WS_D; p.key_source = CSR_KEYS_VALUES; p.key_shift = 32; p.key_mask = 0xFFFFFFFFull; }
        else if (p.kid_in_words) { p.key_source = CSR_KEYS_WORDS; p.key_shift = h.pb + 2; p.key_mask = (1ull << h.nb) - 1; }
        p.rewrite_pairs = in.Z > 0 && !(p.pre_pairs && !in.windowed);
        p.recount = pre;      // (the producer has counted the products of the whole matrix: k_csc_to_csr_keys counts the window's)
    }
    return p;
}

// ---- a row entry --------------------------------------------------------------------------------------------------------------------------------
// a_csr entry = kid << 32 | pos (plain), kid << 32 | hint << 30 | pos (hints), kid << 32 | L << 23 | place << 16 | pos (dense), and with inline partners an
// entry with bit 63 set is 1 << 63 | (partner >> 1) << 32 | posQ | posT << 16.  The numbers are ELBA_CSR_* of include/elba_amd.h (capi.hip asserts it).
enum CsrFormat { CSR_FORMAT_PLAIN = 0, CSR_FORMAT_HINTS = 1, CSR_FORMAT_DENSE = 2, CSR_FORMAT_INLINE = 3 };
ELBA_HD constexpr uint32_t csr_pos_mask(bool suffix, bool hints) { return suffix ? 0xFFFFu : (hints ? 0x3FFFFFFFu : 0xFFFFFFFFu); }
constexpr CsrFormat csr_format(bool inl, bool suffix, bool hints) { return inl ? CSR_FORMAT_INLINE : (suffix ? CSR_FORMAT_DENSE : (hints ? CSR_FORMAT_HINTS : CSR_FORMAT_PLAIN)); }

// the sort word of an entry that carries its one pair: flag | read << rs | (partner >> 1) << 2 pbi | posQ << pbi | posT (both positions below 2^pbi)
ELBA_HD inline uint64_t csr_inline_word(uint64_t read, int rs, uint64_t partner, int pbi, uint64_t posQ, uint64_t posT)
{
    return (1ull << 63) | (read << rs) | ((partner >> 1) << (2 * pbi)) | (posQ << pbi) | posT;
}
// a sorted word -> the row entry.  pbi 0: no word is an inline partner, and bit 63 belongs to the read when the fields fill all 64 bits
ELBA_HD inline uint64_t csr_entry_of_word(uint64_t w, int idbits, int pb, int mb, int pbi)
{
    if (pbi && (w >> 63)) {
        const uint64_t pm = (1ull << pbi) - 1;
        return (1ull << 63) | (((w >> (2 * pbi)) & ((1ull << (mb - 1)) - 1)) << 32) | ((w >> pbi) & pm) | ((w & pm) << 16);
    }
    return (((w >> (pb + 2)) & ((1ull << idbits) - 1)) << 32) | (((w >> pb) & 3ull) << 30) | (w & ((1ull << pb) - 1));
}

}  // namespace elba
