// test_csr_plan — walks the decisions of the CSR build of A (csrc/csr_plan.hpp) without the library: the sort-key layout of the three producers and the
// build's plan against the rules as they stood before the header existed (written out once below, straight-line), that the fields of a key never
// overlap, that the build accepts what every producer of the library hands it, the inline word's encode / decode round trip at the widest and narrowest
// fields, the position mask and format of a row entry, and the column store's geometry.
// The grid (mb 1..32, nb 1..32, pb 1..33, the options, the producer kinds, windowed or not, the longest column) is walked as products that a test can afford:
//   layouts: every (mb, nb, pb) x every combination of the six options a layout reads x everything a producer can know;
//   plans:   every (mb, nb, pb) x every producer x windowed x {4, 17} entries in the longest column x (no option, each option alone), and
//            the widths at which a decision changes x every producer x windowed x every longest column x EVERY combination of the ten options.
// Prints one line per failed check and "ok <checks>" at the end (tests/test_csr_plan_cpu.py reads it); exit status 1 if a check failed.
#include "../csrc/csr_plan.hpp"
#include <cstdio>
#include <random>

using namespace elba;

static long long g_checks = 0, g_failed = 0;
#define CHECK(cond, ...) do { ++g_checks; if (!(cond)) { if (++g_failed <= 40) { printf("FAILED %s:%d %s | ", __FILE__, __LINE__, #cond); printf(__VA_ARGS__); printf("\n"); } } } while (0)

// ---- the rules before csr_plan.hpp: three fragments, copied --------------------------------------------------------------------------------
struct OldPre { bool ready = false, words = false, hints = false, hints_done = false, ell_done = false, inl = false, inline_pending = false, pairs = false; int rs = 0, pbi = 0, nb = 0, pb = 0; uint64_t maxpos = 0; };

// kmer.hip, runs_to_columns (the producer of k_runs_emit): no column seen yet, UPPER instead
static OldPre old_sort_producer(int mb, int nb, int pb, int64_t N, uint64_t maxpos, uint32_t upper, const CsrOptions &o)
{
    const bool words = mb + nb + pb + 2 <= 64 && !o.csr_pairs;
    const bool hints = pb <= 30 && !o.no_hints;
    int rs = nb + pb + 2, pbi = 0;
    bool inl = words && hints && maxpos < 65536 && upper <= 16 && !o.no_pay && !o.no_inline && !o.no_symmetry && !o.no_ell && N < (1ll << 31) && mb >= 2;
    if (inl) {
        const int rs2 = 63 - mb;
        pbi = std::min(pb, (rs2 - (mb - 1)) / 2);
        if (rs2 >= rs && pbi >= 10) rs = rs2; else inl = false;
    }
    OldPre p;
    p.ready = true; p.words = words; p.hints = hints; p.nb = nb; p.pb = pb; p.maxpos = maxpos; p.rs = rs; p.inl = false; p.inline_pending = inl; p.pbi = inl ? pbi : 0;
    return p;
}
// kmer_msd.hip, layout_output + finish (the bucket kernels; pairs_ok: what else the stage asks before it writes a dense matrix's pairs itself)
static OldPre old_msd_producer(int mb, int nb, int pb, int64_t N, uint64_t maxpos, bool use_ell, int64_t max_col, bool pairs_ok, const CsrOptions &o)
{
    const bool words = mb + nb + pb + 2 <= 64 && !o.csr_pairs;
    const bool hints = pb <= 30 && !o.no_hints;
    const bool dense = use_ell && maxpos < 65536 && max_col > 16 && !o.no_pay && !o.no_suffix;
    int rs = nb + pb + 2, pbi = 0;
    bool inl = words && hints && use_ell && !dense && maxpos < 65536 && !o.no_pay && !o.no_inline && !o.no_symmetry && N < (1ll << 31) && mb >= 2;
    if (inl) {
        const int rs2 = 63 - mb;
        pbi = std::min(pb, (rs2 - (mb - 1)) / 2);
        if (rs2 >= rs && pbi >= 10) rs = rs2; else inl = false;
    }
    OldPre p;
    p.ready = true; p.words = words; p.hints = hints; p.hints_done = hints && words; p.ell_done = true; p.inline_pending = false;
    p.nb = nb; p.pb = pb; p.maxpos = maxpos; p.rs = rs; p.inl = inl; p.pbi = inl ? pbi : 0;      // (the stage kept a pbi it did not use: nobody read it)
    p.pairs = dense && pairs_ok;
    return p;
}
static int old_bits(uint64_t maxval) { int b = 1; while (b < 64 && (maxval >> b)) ++b; return b; }

// matrix.hip, finish_matrix_from_sorted_csc: every decision, in the order it made them
struct OldPlan {
    bool pos16 = false, suffix = false, hints = false, one_word = false, row_order = false; uint32_t j_shift = 5;
    int mismatch = 0;
    bool have_words = false, inl_here = false, inl_late = false, write_words = false, add_hints = false, fin = false, csr_inline = false, inline_window = false;
    int rs = 0, pbi = 0, idbits = 0, pbi_used = 0, write_pbi = 0, add_pbi = 0;
    bool pre_pairs = false, kid_in_words = false, rewrite = false, recount = false; int k0 = 0, k1 = 2, spare = 1, ks = -1; uint64_t km = ~0ull;
};
static OldPlan old_plan(int64_t M, int64_t N, int64_t Z, uint64_t maxpos, bool windowed, bool use_ell, bool ell_compact, int64_t max_col, const OldPre *prep, const CsrOptions &o)
{
    OldPlan p;
    const bool pre = prep != nullptr;
    const OldPre none, &h = pre ? *prep : none;
    p.pos16 = maxpos < 65536;
    const int mb = old_bits((uint64_t)(M > 0 ? M - 1 : 0)), nb = old_bits((uint64_t)(N > 0 ? N - 1 : 0)), pb = old_bits(maxpos);
    bool hints = pre ? h.hints : (pb <= 30 && !o.no_hints);
    p.suffix = use_ell && p.pos16 && max_col > 16 && !o.no_pay && !o.no_suffix;
    if (p.suffix) { hints = false; p.j_shift = max_col <= 32 ? 5u : 6u; }
    p.one_word = !p.suffix && mb + nb + pb + 2 <= 64 && !o.csr_pairs;
    if (p.one_word) {
        const bool have_words = p.have_words = pre && h.words && h.nb == nb && h.pb == pb;
        if (!(!pre || have_words)) p.mismatch = 1;
        int rs = have_words ? h.rs : nb + pb + 2, pbi = have_words ? h.pbi : 0;
        bool inl_here = false;
        if (!have_words && hints && use_ell && p.pos16 && !o.no_pay && !o.no_inline && !o.no_symmetry && (!windowed || o.panel_inline) && N < (1ll << 31) && mb >= 2) {
            const int rs2 = 63 - mb, pbi2 = std::min(pb, (rs2 - (mb - 1)) / 2);
            if (rs2 >= nb + pb + 2 && pbi2 >= 10) { rs = rs2; pbi = pbi2; inl_here = true; }
        }
        p.write_words = Z > 0 && !have_words; p.write_pbi = inl_here ? pbi : 0;
        const bool inl_late = have_words && hints && !h.hints_done && h.inline_pending && use_ell && !p.suffix && p.pos16 && !windowed;
        p.add_hints = Z > 0 && have_words && hints && !h.hints_done; p.add_pbi = inl_late ? pbi : 0;
        p.idbits = have_words && ell_compact ? std::min(32, rs - pb - 2) : nb;
        p.pbi_used = (have_words && h.inl) || inl_here || inl_late ? pbi : 0;
        p.fin = Z > 0 && M > 0 && o.tune1 != 1;
        p.csr_inline = (have_words && h.inl) || inl_here || inl_late;
        p.inline_window = inl_here && windowed;
        p.rs = rs; p.pbi = pbi; p.inl_here = inl_here; p.inl_late = inl_late;
    } else {
        const bool pre_pairs = p.pre_pairs = pre && h.pairs;
        if (!(!pre || !h.words || p.suffix || pre_pairs)) p.mismatch = 1;
        else if (!(!pre_pairs || p.suffix)) p.mismatch = 2;
        const bool kid_in_words = p.kid_in_words = pre && h.words && !pre_pairs;
        p.k0 = pre_pairs ? 1 : 0; p.k1 = pre_pairs ? 0 : 2; p.spare = pre_pairs ? 3 : 1;
        p.ks = pre_pairs ? 32 : kid_in_words ? h.pb + 2 : -1;
        p.km = pre_pairs ? 0xFFFFFFFFull : kid_in_words ? (1ull << h.nb) - 1 : ~0ull;
        p.rewrite = Z > 0 && !(pre_pairs && !windowed); p.recount = pre;
    }
    p.hints = hints;
    p.row_order = p.suffix && !o.no_row_order && M > 1 && Z > 0;
    return p;
}

// ---- the walk ------------------------------------------------------------------------------------------------------------------------------------
static CsrHandoff handoff_of(const OldPre &p)
{
    CsrHandoff h;
    h.state = CsrHandoff::READY; h.words = p.words; h.hints = p.hints; h.hints_done = p.hints_done; h.ell_done = p.ell_done; h.inl = p.inl; h.inline_pending = p.inline_pending; h.pairs = p.pairs;
    h.rs = p.rs; h.pbi = p.pbi; h.nb = p.nb; h.pb = p.pb; h.maxpos = p.maxpos;
    return h;
}
static bool same_handoff(const CsrHandoff &a, const CsrHandoff &b)
{
    return a.state == b.state && a.words == b.words && a.hints == b.hints && a.hints_done == b.hints_done && a.ell_done == b.ell_done && a.inl == b.inl && a.inline_pending == b.inline_pending &&
           a.pairs == b.pairs && a.rs == b.rs && a.pbi == b.pbi && a.nb == b.nb && a.pb == b.pb && a.maxpos == b.maxpos;
}
static CsrOptions options_of(unsigned bits)
{
    CsrOptions o;
    o.csr_pairs = bits & 1; o.no_hints = bits & 2; o.no_pay = bits & 4; o.no_inline = bits & 8; o.no_symmetry = bits & 16; o.panel_inline = bits & 32;
    o.no_ell = bits & 64; o.no_suffix = bits & 128; o.no_row_order = bits & 256; o.tune1 = bits & 512 ? 1 : 0;
    return o;
}
// sizes whose largest index / position needs exactly that many bits
static int64_t count_of_bits(int b) { return b == 1 ? 2 : (1ll << (b - 1)) + 1; }
static uint64_t maxpos_of_bits(int b) { return b == 1 ? 1 : 1ull << (b - 1); }

static void check_fields(const char *what, int mb, int nb, int pb, bool words, int rs, int pbi, bool inl)
{
    CHECK(rs >= nb + pb + 2, "%s mb %d nb %d pb %d: rs %d", what, mb, nb, pb, rs);
    if (words) CHECK(rs + mb <= 64, "%s mb %d nb %d pb %d: rs %d", what, mb, nb, pb, rs);
    if (inl) CHECK(rs == 63 - mb && (mb - 1) + 2 * pbi <= rs && pbi >= 10 && pbi <= pb, "%s mb %d nb %d pb %d: rs %d pbi %d", what, mb, nb, pb, rs, pbi);
    else CHECK(pbi == 0, "%s mb %d nb %d pb %d: pbi %d without inline partners", what, mb, nb, pb, pbi);
}

enum Producer { P_NONE, P_SORT, P_MSD, P_MSD_PAIRS_LATE, P_COUNT };

static void walk_plan(int mb, int nb, int pb, unsigned optbits, int producer, bool windowed, int64_t max_col)
{
    const CsrOptions o = options_of(optbits);
    const int64_t M = count_of_bits(mb), N = count_of_bits(nb), Z = N + 1;
    const uint64_t maxpos = maxpos_of_bits(pb);
    const bool use_ell = !o.no_ell && max_col <= 64;
    OldPre op; CsrHandoff h;
    bool compact = false;
    if (producer == P_SORT) {
        if (windowed) return;      // (the k-mer stage builds whole matrices)
        op = old_sort_producer(mb, nb, pb, N, maxpos, (uint32_t)max_col, o);
        h = csr_handoff(csr_key_layout(mb, nb, pb, N, o, CsrProducer{!o.no_ell, max_col <= CSR_SPARSE_MAX_COL, maxpos < 65536, false}, CSR_INLINE_PENDING), nb, pb, maxpos);
    } else if (producer != P_NONE) {
        if (windowed) return;
        op = old_msd_producer(mb, nb, pb, N, maxpos, use_ell, max_col, producer == P_MSD, o);
        const bool dense = csr_dense(use_ell, maxpos < 65536, max_col, o);
        const CsrKeyLayout l = csr_key_layout(mb, nb, pb, N, o, CsrProducer{use_ell, !dense, maxpos < 65536, false}, CSR_INLINE_NOW);
        h = csr_handoff(l, nb, pb, maxpos);
        h.hints_done = l.hints && l.words; h.ell_done = true; h.pairs = dense && producer == P_MSD;
        compact = l.inl == CSR_INLINE_NOW && l.words && use_ell;
    }
    if (producer != P_NONE) {
        CHECK(same_handoff(h, handoff_of(op)), "producer %d mb %d nb %d pb %d options %x longest column %lld: the hand-off", producer, mb, nb, pb, optbits, (long long)max_col);
        check_fields("hand-off", mb, nb, pb, h.words, h.rs, h.pbi, h.inl || h.inline_pending);
    }
    CsrBuildInput in;
    in.M = M; in.N = N; in.Z = Z; in.maxpos = maxpos; in.windowed = windowed; in.use_ell = use_ell; in.ell_compact = compact; in.max_col = max_col; in.pre = producer == P_NONE ? nullptr : &h; in.opt = o;
    const CsrBuildPlan p = plan_csr_build(in);
    const OldPlan q = old_plan(M, N, Z, maxpos, windowed, use_ell, compact, max_col, producer == P_NONE ? nullptr : &op, o);
#define WHERE "producer %d mb %d nb %d pb %d options %x windowed %d longest column %lld", producer, mb, nb, pb, optbits, (int)windowed, (long long)max_col
    // producer and consumer agree: the build takes what the library's own producers leave
    CHECK(p.mismatch == CSR_MATCH && q.mismatch == 0, WHERE);
    if (producer != P_NONE && h.words && p.one_word) CHECK(p.have_words, WHERE);
    CHECK(p.mb == mb && p.nb == nb && p.pb == pb, WHERE);
    CHECK(p.pos16 == q.pos16 && p.suffix == q.suffix && p.hints == q.hints && p.one_word == q.one_word && p.row_order == q.row_order && (!p.suffix || p.j_shift == q.j_shift), WHERE);
    if (p.one_word) {
        CHECK(p.have_words == q.have_words && p.write_words == q.write_words && p.add_hints == q.add_hints && p.fin_sort == q.fin, WHERE);
        CHECK(p.rs == q.rs && p.idbits == q.idbits && p.pbi_used == q.pbi_used && p.write_pbi == q.write_pbi && p.add_pbi == q.add_pbi, WHERE);
        CHECK((p.inl != CSR_INL_NONE ? p.pbi : 0) == (q.csr_inline ? q.pbi : 0), WHERE);
        CHECK((p.inl == CSR_INL_HERE) == q.inl_here && (p.inl == CSR_INL_LATE) == q.inl_late && (p.inl == CSR_INL_WORDS) == (q.have_words && op.inl) && (p.inl != CSR_INL_NONE) == q.csr_inline && p.inline_window == q.inline_window, WHERE);
        check_fields("plan", mb, nb, pb, true, p.rs, p.pbi_used, p.inl != CSR_INL_NONE);
        CHECK(p.idbits >= 1 && p.idbits <= 32 && p.pb + 2 + p.idbits <= p.rs, WHERE);
    } else {
        CHECK(p.pre_pairs == q.pre_pairs && p.kid_in_words == q.kid_in_words && p.rewrite_pairs == q.rewrite && p.recount == q.recount, WHERE);
        CHECK((int)p.k0 == q.k0 && (int)p.k1 == q.k1 && (int)p.spare == q.spare && p.key_shift == q.ks && p.key_mask == q.km, WHERE);
        CHECK(p.key_source == (q.pre_pairs ? CSR_KEYS_VALUES : q.kid_in_words ? CSR_KEYS_WORDS : CSR_KEYS_CALLER) && p.inl == CSR_INL_NONE && !p.inline_window, WHERE);
    }
#undef WHERE
}

static void walk_layouts_and_plans()
{
    const int64_t cols[] = {1, 4, 5, 16, 17, 32, 33, 64, 65, 127, 128};
    for (int mb = 1; mb <= 32; ++mb)
        for (int nb = 1; nb <= 32; ++nb)
            for (int pb = 1; pb <= 33; ++pb) {
                const int64_t N = count_of_bits(nb);
                const uint64_t maxpos = maxpos_of_bits(pb);
                // layouts: the six options a layout reads, everything a producer can know
                for (unsigned ob = 0; ob < 64; ++ob) {
                    const CsrOptions o = options_of(ob);
                    for (unsigned k = 0; k < 8; ++k) {
                        const CsrProducer pr{(k & 1) != 0, (k & 2) != 0, maxpos < 65536, (k & 4) != 0};
                        const CsrKeyLayout l = csr_key_layout(mb, nb, pb, N, o, pr, CSR_INLINE_NOW);
                        // (one fragment, with what each producer knew in its place: UPPER <= 16 / !dense / the one-word branch for "not dense", !no_ell / use_ell for "padded", no window but in matrix.hip)
                        const bool words = mb + nb + pb + 2 <= 64 && !o.csr_pairs, hints = pb <= 30 && !o.no_hints;
                        int rs = nb + pb + 2, pbi = 0;
                        bool inl = words && hints && pr.padded && pr.not_dense && pr.pos16 && !o.no_pay && !o.no_inline && !o.no_symmetry && (!pr.windowed || o.panel_inline) && N < (1ll << 31) && mb >= 2;
                        if (inl) { const int rs2 = 63 - mb; pbi = std::min(pb, (rs2 - (mb - 1)) / 2); if (rs2 >= rs && pbi >= 10) rs = rs2; else { inl = false; pbi = 0; } }
                        CHECK(l.words == words && l.hints == hints && l.rs == rs && l.pbi == pbi && (l.inl == CSR_INLINE_NOW) == inl && (l.inl == CSR_INLINE_NONE) == !inl, "layout mb %d nb %d pb %d options %x producer %x", mb, nb, pb, ob, k);
                        check_fields("layout", mb, nb, pb, l.words, l.rs, l.pbi, l.inl != CSR_INLINE_NONE);
                    }
                }
                // plans: every width, no option and each option alone
                for (int producer = 0; producer < P_COUNT; ++producer)
                    for (int windowed = 0; windowed < 2; ++windowed)
                        for (int64_t mc : {(int64_t)4, (int64_t)17}) {
                            walk_plan(mb, nb, pb, 0, producer, windowed != 0, mc);
                            for (unsigned b = 0; b < 10; ++b) walk_plan(mb, nb, pb, 1u << b, producer, windowed != 0, mc);
                        }
            }
    // plans: every combination of the options, at the widths where a decision changes — one row; a row id of 2 bits (the first with a partner field); the widest
    // read that leaves 16 and 10 position bits, and one bit more; 32 bits; positions of 10, 16, 17, 30, 31 bits; then words of 64 and 65 bits
    const int mbs[] = {1, 2, 16, 22, 23, 32}, nbs[] = {1, 20, 32}, pbs[] = {1, 10, 16, 17, 30, 31};
    for (int mb : mbs)
        for (int nb : nbs)
            for (int pb : pbs)
                for (unsigned ob = 0; ob < 1024; ++ob)
                    for (int producer = 0; producer < P_COUNT; ++producer)
                        for (int windowed = 0; windowed < 2; ++windowed)
                            for (int64_t mc : cols) walk_plan(mb, nb, pb, ob, producer, windowed != 0, mc);
    for (int mb = 1; mb <= 32; ++mb)      // words of exactly 64 bits and one more
        for (int pb : {10, 16, 30})
            for (int extra = 0; extra < 2; ++extra) {
                const int nb = 62 + extra - mb - pb;
                if (nb < 1 || nb > 32) continue;
                for (unsigned ob = 0; ob < 1024; ++ob)
                    for (int producer = 0; producer < P_COUNT; ++producer) walk_plan(mb, nb, pb, ob, producer, false, 8);
            }
}

// a mismatch is reported, not built: what another matrix's hand-off (or options changed between the two calls) does
static void walk_mismatches()
{
    const CsrOptions o;
    const int mb = 11, nb = 16, pb = 12;
    CsrBuildInput in;
    in.M = count_of_bits(mb); in.N = count_of_bits(nb); in.Z = 100; in.maxpos = maxpos_of_bits(pb); in.use_ell = true; in.max_col = 8; in.opt = o;
    CsrHandoff h = csr_handoff(csr_key_layout(mb, nb, pb, in.N, o, CsrProducer{true, true, true, false}, CSR_INLINE_PENDING), nb, pb, in.maxpos);
    in.pre = &h;
    CHECK(plan_csr_build(in).mismatch == CSR_MATCH && plan_csr_build(in).have_words && plan_csr_build(in).inl == CSR_INL_LATE, "the sort path's own hand-off");
    h.nb = nb + 1; CHECK(plan_csr_build(in).mismatch == CSR_WORDS_DO_NOT_MATCH, "another nb"); h.nb = nb;
    h.pb = pb - 1; CHECK(plan_csr_build(in).mismatch == CSR_WORDS_DO_NOT_MATCH, "another pb"); h.pb = pb;
    h.words = false; CHECK(plan_csr_build(in).mismatch == CSR_WORDS_DO_NOT_MATCH, "no words for a one-word build"); h.words = true;
    in.opt.csr_pairs = true; CHECK(plan_csr_build(in).mismatch == CSR_WORDS_DO_NOT_MATCH, "words for a pair build that is not dense"); in.opt.csr_pairs = false;
    h.pairs = true; h.words = false; in.opt.csr_pairs = true; CHECK(plan_csr_build(in).mismatch == CSR_PAIRS_NOT_DENSE, "a dense matrix's pairs, the matrix is not one");
    in.opt.csr_pairs = false; in.max_col = 20; CHECK(plan_csr_build(in).mismatch == CSR_MATCH && plan_csr_build(in).suffix && plan_csr_build(in).pre_pairs, "a dense matrix's pairs");
    CsrHandoff used = h; used.consume();
    CHECK(used.state == CsrHandoff::CONSUMED && !used.ready() && !used.words && !used.pairs, "consume");
    in.pre = &used; CHECK(plan_csr_build(in).mismatch == CSR_MATCH && !plan_csr_build(in).pre_pairs && plan_csr_build(in).key_source == CSR_KEYS_CALLER, "a consumed hand-off is none");
    CHECK(CsrHandoff{}.state == CsrHandoff::NONE && !CsrHandoff{}.ready(), "default");
}

static void walk_round_trips()
{
    std::mt19937_64 rng(12345);
    auto below = [&](int bits) { return bits >= 64 ? rng() : rng() & ((1ull << bits) - 1); };
    // inline partners at the extreme widths a layout admits: pbi 10 with reads of 2 and of 22 bits, pbi 16 with reads of 2 and of 16 bits
    struct { int mb, nb, pb; } inl[] = {{2, 31, 10}, {22, 8, 10}, {2, 20, 16}, {16, 12, 16}, {2, 31, 28}, {11, 16, 14}};
    for (auto &w : inl) {
        const CsrKeyLayout l = csr_key_layout(w.mb, w.nb, w.pb, count_of_bits(w.nb), CsrOptions{}, CsrProducer{true, true, true, false}, CSR_INLINE_NOW);
        CHECK(l.inl == CSR_INLINE_NOW && l.rs == 63 - w.mb, "mb %d nb %d pb %d: inline partners", w.mb, w.nb, w.pb);
        for (int t = 0; t < 20000; ++t) {
            const uint64_t read = below(w.mb), partner = below(w.mb), posQ = t == 0 ? (1ull << l.pbi) - 1 : below(l.pbi), posT = t == 1 ? (1ull << l.pbi) - 1 : below(l.pbi);
            const uint64_t word = csr_inline_word(read, l.rs, partner, l.pbi, posQ, posT);
            CHECK((word >> 63) == 1 && ((word >> l.rs) & ((1ull << w.mb) - 1)) == read, "mb %d pbi %d: the read of an inline word", w.mb, l.pbi);
            const uint64_t e = csr_entry_of_word(word, w.nb, w.pb, w.mb, l.pbi);
            CHECK(e == ((1ull << 63) | ((partner >> 1) << 32) | posQ | (posT << 16)), "mb %d pbi %d: read %llu partner %llu posQ %llu posT %llu -> %llx", w.mb, l.pbi, (unsigned long long)read,
                  (unsigned long long)partner, (unsigned long long)posQ, (unsigned long long)posT, (unsigned long long)e);
            // a word of the same layout that names its k-mer: flag clear
            const uint64_t kid = below(w.nb), hint = below(2), pos = below(w.pb);
            const uint64_t plain = (read << l.rs) | (kid << (w.pb + 2)) | (hint << w.pb) | pos;
            CHECK(csr_entry_of_word(plain, w.nb, w.pb, w.mb, l.pbi) == ((kid << 32) | (hint << 30) | pos), "mb %d pbi %d: a plain word beside inline ones", w.mb, l.pbi);
        }
    }
    // reads of 23 bits and more leave no room for inline partners; at 31 bits the plain word round-trips, also when read, id, hints and position fill
    // all 64 bits: bit 63 is then the read's top bit and pbi is 0
    for (int mb = 23; mb <= 32; ++mb)
        for (int pb = 10; pb <= 16; ++pb) CHECK(csr_key_layout(mb, 8, pb, 200, CsrOptions{}, CsrProducer{true, true, true, false}, CSR_INLINE_NOW).inl == CSR_INLINE_NONE, "mb %d pb %d: no room", mb, pb);
    struct { int mb, nb, pb; } full[] = {{31, 20, 11}, {31, 1, 30}, {32, 20, 10}, {2, 32, 28}, {31, 10, 10}};
    for (auto &w : full) {
        const CsrKeyLayout l = csr_key_layout(w.mb, w.nb, w.pb, count_of_bits(w.nb), CsrOptions{}, CsrProducer{true, true, true, false}, CSR_INLINE_NOW);
        CHECK(l.words && l.pbi == 0 && l.rs == w.nb + w.pb + 2, "mb %d nb %d pb %d: plain words", w.mb, w.nb, w.pb);
        for (int t = 0; t < 20000; ++t) {
            const uint64_t read = t == 0 ? (1ull << w.mb) - 1 : below(w.mb), kid = below(w.nb), hint = below(2), pos = below(w.pb);
            const uint64_t word = (read << l.rs) | (kid << (w.pb + 2)) | (hint << w.pb) | pos;
            CHECK(((word >> l.rs) & ((1ull << w.mb) - 1)) == read && csr_entry_of_word(word, w.nb, w.pb, w.mb, 0) == ((kid << 32) | (hint << 30) | pos), "mb %d nb %d pb %d: the plain word", w.mb, w.nb, w.pb);
        }
    }
}

static void walk_entry_format()
{
    CHECK(csr_pos_mask(true, false) == 0xFFFFu && csr_pos_mask(true, true) == 0xFFFFu && csr_pos_mask(false, true) == (1u << 30) - 1 && csr_pos_mask(false, false) == ~0u, "position masks");
    for (int b = 0; b < 8; ++b) {
        const bool inl = b & 1, suffix = b & 2, hints = b & 4;
        CHECK((int)csr_format(inl, suffix, hints) == (inl ? 3 : suffix ? 2 : hints ? 1 : 0), "format %d", b);
    }
    static_assert(CSR_FORMAT_PLAIN == 0 && CSR_FORMAT_HINTS == 1 && CSR_FORMAT_DENSE == 2 && CSR_FORMAT_INLINE == 3, "the ABI's numbers");
    CHECK(bits_needed(0) == 1 && bits_needed(1) == 1 && bits_needed(2) == 2 && bits_needed(65535) == 16 && bits_needed(65536) == 17 && bits_needed(~0ull) == 64 && bits_needed_u(255) == 8, "bit widths");
    for (int b = 1; b < 64; ++b) CHECK(bits_needed((1ull << b) - 1) == b && bits_needed(1ull << b) == b + 1 && old_bits(1ull << b) == b + 1, "bit width %d", b);
}

static void walk_column_store()
{
    const size_t big = (size_t)1 << 45;
    for (int64_t mc : {0ll, 1ll, 4ll, 5ll, 8ll, 9ll, 16ll, 17ll, 32ll, 33ll, 40ll, 64ll, 65ll, 127ll, 128ll, 100000ll})
        for (int no_ell = 0; no_ell < 2; ++no_ell)
            for (int64_t N : {0ll, 1ll, 1000ll, 60041ll}) {
                const ColumnStore s = plan_column_store(N, mc, no_ell != 0, big);
                // matrix.hip, choose_column_store as it stood
                const uint32_t m = (uint32_t)(mc > 0 ? mc : 1), stride = m <= 4 ? 4u : (m + 7u) & ~7u;
                const bool use_ell = m <= 64 && N > 0 && !no_ell && (size_t)N * stride * 8 <= big / 3 && (uint64_t)N * stride < (1ull << 40);
                uint32_t lb = 1, fbits = 0, s_stride = 0;
                if (use_ell) { uint32_t fb = 2; while ((2u << lb) < stride) ++lb; while ((1u << fb) < stride) ++fb; s_stride = stride; fbits = fb; }
                else { while (lb < 6 && (2u << lb) < m) ++lb; int fb = 1; while (fb < 31 && ((uint64_t)(m > 1 ? m - 1 : 1) >> fb)) ++fb; fbits = (uint32_t)fb; }
                CHECK(s.padded == use_ell && s.stride == s_stride && s.lpc_log2 == lb && s.fbits == fbits && s.bytes == (size_t)N * stride * 8, "longest column %lld, N %lld, no_ell %d", (long long)mc, (long long)N, no_ell);
                CHECK(column_stride(m) == stride && (m <= 4 ? stride == 4 : stride % 8 == 0 && stride >= m && stride < m + 8), "stride of %u", m);
                if (s.padded) CHECK((2u << s.lpc_log2) >= s.stride && (1u << s.fbits) >= s.stride && s.stride >= m, "padded geometry of %u", m);
                else CHECK(s.stride == 0 && (m <= 1 || (1u << s.fbits) >= m) && s.lpc_log2 >= 1 && s.lpc_log2 <= 6, "plain geometry of %u", m);
            }
    { const ColumnStore a = plan_column_store(1000, 8, false, 3 * 64000), b = plan_column_store(1000, 8, false, 3 * 64000 - 1);
      CHECK(a.padded && a.wanted && !b.padded && b.wanted && b.bytes == 64000, "a third of the free memory"); }
    { const ColumnStore a = plan_column_store((1ll << 37) - 1, 8, false, ~(size_t)0), b = plan_column_store(1ll << 37, 8, false, ~(size_t)0);
      CHECK(a.padded && !b.padded && b.wanted, "2^40 slots"); }
    { const ColumnStore g4 = plan_column_store(9, 4, false, big), g8 = plan_column_store(9, 8, false, big), g16 = plan_column_store(9, 16, false, big), g40 = plan_column_store(9, 40, false, big);
      CHECK(g4.stride == 4 && g4.lpc_log2 == 1 && g4.fbits == 2 && g8.stride == 8 && g8.lpc_log2 == 2 && g8.fbits == 3 && g16.stride == 16 && g16.lpc_log2 == 3 && g16.fbits == 4 && g40.stride == 40 && g40.lpc_log2 == 5 && g40.fbits == 6, "the literals"); }
    CHECK(!csr_dense(true, true, 16, CsrOptions{}) && csr_dense(true, true, 17, CsrOptions{}) && !csr_dense(false, true, 17, CsrOptions{}) && !csr_dense(true, false, 17, CsrOptions{}), "dense");
    { CsrOptions o; o.no_pay = true; CHECK(!csr_dense(true, true, 17, o), "no_pay"); o = CsrOptions{}; o.no_suffix = true; CHECK(!csr_dense(true, true, 17, o), "no_suffix"); }
}

int main()
{
    walk_entry_format();
    walk_column_store();
    walk_round_trips();
    walk_mismatches();
    walk_layouts_and_plans();
    if (g_failed) { printf("%lld of %lld checks failed\n", g_failed, g_checks); return 1; }
    printf("ok %lld\n", g_checks);
    return 0;
}
