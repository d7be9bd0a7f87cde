// test_ov_plan — walks csrc/ov_plan.hpp without the library: the plan of the overlap SpGEMM's host driver on named shapes and on a few thousand random
// ones, field by field against a verbatim copy of the expressions the driver held before the plan existed (old_plan: one function, as
// create_seed_matrix_direct and ov_launch_finalize computed them), the properties every plan must have, the repeated pass and the hint updates.
// Prints one line per failed check and "ok <checks>" at the end (tests/test_ov_plan_cpu.py reads it); exit status 1 if a check failed.
#include "../csrc/ov_plan.hpp"
#include <cstdio>
#include <random>
#include <string>

using namespace elba;

static int g_checks = 0, g_failed = 0;
#define CHECK(cond, ...) do { ++g_checks; if (!(cond)) { ++g_failed; printf("FAILED %s:%d %s | ", __FILE__, __LINE__, #cond); printf(__VA_ARGS__); printf("\n"); } } while (0)

// ---- the old expressions ------------------------------------------------------------------------------------------------------------------
// `c` reads like the context did; what the old driver kept in locals and in OvParams is kept in fields of the same names
struct OldLaunch { bool launched = false; int B = 0; bool G = false, P = false, S = false; int TBC = 0; long long grid = 0; size_t lds = 0; int tier = 0; unsigned tb = 0; bool spec = false; int dk = 0; };
struct OldPlan {
    uint64_t gstride; int spill_blocks; bool half; int64_t slack, ov_tmp_cap, b_cap_entries;
    uint32_t p_half, pos_mask, hint_mask, suffix, inl, prior_q16, use_feedback, pay16, qblk_log2, min_tier, max_col, tier_limit[5], nsample, sstep, slab_prior_q16, slab_pct;
    bool row_order, ov_hints_used, pay, mir16, sampling, ov_slab_on, spec; int64_t ov_slab_cap; unsigned long long fb_enough;
    int tmax, dk, classify_nb; uint32_t skipped_tiers;
    OldLaunch sample, tier[6];
    // ov_launch_finalize
    bool fin_slab, scan, narrow; long long slab_fold_nb, rp_nb, fin_nb, bucket_nb; uint64_t sstride; uint32_t skipped_sorts; bool bucket, huge;
};
struct OldCtx {
    int64_t M, N, Z, row_lo, row_hi, max_row_nnz, max_col_nnz; uint32_t fbits; bool pos16, use_ell, csr_hints, csr_inline, csr_suffix, have_row_order; int num_cus;
    struct { bool no_symmetry, no_pay, mir32, no_slab, no_sample, ov_generic; int dk, dense_up, dense_wgs, slab_q16, slab_pct; int64_t tune[8]; } opt;
    uint32_t ov_prior_q16, ov_slab_q16; bool ov_tiers_known, ov_tier_used[8], ov_sort_used[2];
    int64_t ov_tmp_cap; struct { int64_t workspace_hint_bytes; } cfg;
};
static OldCtx old_ctx(const OvInput &in)
{
    OldCtx c{};
    c.M = in.M; c.N = in.N; c.Z = in.Z; c.row_lo = in.row_lo; c.row_hi = in.row_hi; c.max_row_nnz = in.max_row_nnz; c.max_col_nnz = in.max_col_nnz; c.fbits = in.fbits;
    c.pos16 = in.pos16; c.use_ell = in.use_ell; c.csr_hints = in.csr_hints; c.csr_inline = in.csr_inline; c.csr_suffix = in.csr_suffix; c.have_row_order = in.have_row_order; c.num_cus = in.num_cus;
    c.opt.no_symmetry = in.opt.no_symmetry; c.opt.no_pay = in.opt.no_pay; c.opt.mir32 = in.opt.mir32; c.opt.no_slab = in.opt.no_slab; c.opt.no_sample = in.opt.no_sample; c.opt.ov_generic = in.opt.ov_generic;
    c.opt.dk = in.opt.dk; c.opt.dense_up = in.opt.dense_up; c.opt.dense_wgs = in.opt.dense_wgs; c.opt.slab_q16 = in.opt.slab_q16; c.opt.slab_pct = in.opt.slab_pct;
    c.opt.tune[3] = in.opt.tune3; c.opt.tune[4] = in.opt.tune4; c.opt.tune[5] = in.opt.tune5; c.opt.tune[7] = in.opt.tune7;
    c.ov_prior_q16 = in.hints.prior_q16; c.ov_slab_q16 = in.hints.slab_q16; c.ov_tiers_known = in.hints.tiers_known;
    for (int t = 0; t < 6; ++t) c.ov_tier_used[t] = in.hints.tier_used[t];
    c.ov_sort_used[0] = in.hints.sort_used[0]; c.ov_sort_used[1] = in.hints.sort_used[1];
    c.ov_tmp_cap = in.tmp_cap; c.cfg.workspace_hint_bytes = in.workspace_hint_bytes;
    return c;
}

static OldPlan old_plan(const OvInput &in)
{
    const int NUM_LDS_TIERS = 5, NUM_TIERS = 6, LDS_TBITS0 = 9; const uint32_t STAGE_CHUNK = 1024, FIN_WAVE2_MAX = 1024, SLAB_PAD = 16; const int RP_TILE = 1024;
    struct StageRec { uint32_t w[8]; };
    OldCtx c = old_ctx(in);
    const int phase = in.phase, passes = in.pass;
    const size_t free_b = (size_t)in.free_bytes;
    OldPlan o{};
    struct { uint32_t half, pos_mask, hint_mask, suffix, inl, prior_q16, use_feedback, pay16, qblk_log2, min_tier, max_col, Mcols, dense_up, tier_limit[5], nsample, sstep, slab_prior_q16, slab_pct; bool row_order; unsigned long long fb_enough; } p{};
    const int64_t M = c.M, Z = c.Z;
    const int64_t row_lo = c.row_lo, row_hi = c.row_hi;

    uint64_t gstride = 2;
    while (gstride < 2ull * (uint64_t)(M > 1 ? M : 1)) gstride <<= 1;
    int spill_blocks = (int)((4ull << 30) / (20ull * gstride));
    spill_blocks = spill_blocks < 64 ? 64 : (spill_blocks > c.num_cus * 2 ? c.num_cus * 2 : spill_blocks);

    const int cus = c.num_cus;
    const int64_t nrows = row_hi - row_lo;
    const bool half = phase >= 1 || !c.opt.no_symmetry || c.csr_inline;
    const int64_t slack = (int64_t)cus * 32 * STAGE_CHUNK + 64;
    if (c.ov_tmp_cap == 0) {
        if (c.cfg.workspace_hint_bytes > 0) c.ov_tmp_cap = c.cfg.workspace_hint_bytes / (int64_t)sizeof(StageRec);
        else {
            const int64_t budget = (int64_t)(free_b / 2 / (sizeof(StageRec) + (half ? 2 * (24 + 32) : 24)));
            c.ov_tmp_cap = std::min<int64_t>(std::max<int64_t>(half ? Z / 2 : Z, 1 << 16) + slack, std::max<int64_t>(budget, 1024));
        }
        if (c.ov_tmp_cap < 1024) c.ov_tmp_cap = 1024;
    }
    p.dense_up = (uint32_t)c.opt.dense_up;
    p.max_col = (uint32_t)(c.max_col_nnz > 0 ? c.max_col_nnz : 1);
    p.Mcols = (uint32_t)M;
    p.half = phase >= 1 ? 2u : (half ? 1u : 0u);
    p.pos_mask = c.csr_suffix ? 0xFFFFu : (c.csr_hints ? 0x3FFFFFFFu : 0xFFFFFFFFu);
    p.hint_mask = !c.csr_hints ? 0u : (p.half == 2u ? 1u << 30 : (p.half == 1u ? 1u << 31 : 0u));
    p.suffix = c.csr_suffix && p.half == 1u ? 1u : 0u;
    p.inl = c.csr_inline ? 1u : 0u;
    p.row_order = p.suffix && c.have_row_order;
    o.ov_hints_used = p.hint_mask != 0u || p.suffix != 0u || c.csr_inline;
    p.prior_q16 = c.ov_prior_q16 ? c.ov_prior_q16 : 16384u;
    p.use_feedback = c.ov_prior_q16 ? 0u : 1u;
    p.fb_enough = (unsigned long long)std::min<int64_t>(std::max<int64_t>(Z / 32, 1 << 16), 1 << 23);
    bool pay = c.pos16 && !c.opt.no_pay;
    const bool pay16 = pay && c.use_ell && !c.csr_suffix && c.opt.tune[3] != 1 && ((uint64_t)c.max_row_nnz << c.fbits) <= 65536ull;
    p.pay16 = pay16 ? 1u : 0u;
    if (pay16) pay = false;
    const uint32_t blk[5] = {p.suffix ? 256u : 128u, p.suffix && p.dense_up >= 1u ? 512u : 256u, p.suffix && p.dense_up >= 2u ? 1024u : 512u, 1024u, 512u};
    for (int t = 0; t < NUM_LDS_TIERS; ++t) {
        const uint32_t T = 1u << (LDS_TBITS0 + t);
        p.tier_limit[t] = std::min((T >> 2) * 3, T - blk[t]) - 1;
    }
    p.qblk_log2 = c.opt.tune[5] > 0 ? (uint32_t)std::min<int64_t>(c.opt.tune[5] - 1, 12) : 0u;
    p.min_tier = (pay16 && nrows >= 65536 && Z / nrows >= 1024 && c.opt.tune[4] != 1) ? 2u : 0u;
    if (c.opt.tune[7] >= 1 && c.opt.tune[7] <= NUM_TIERS) p.min_tier = (uint32_t)(c.opt.tune[7] - 1);

    // the pass
    const bool mir16 = c.pos16 && !c.opt.mir32;
    o.b_cap_entries = half ? 2 * c.ov_tmp_cap : c.ov_tmp_cap;
    p.use_feedback = c.ov_prior_q16 ? 0u : 1u;
    const bool sampling = p.use_feedback && nrows >= 8192 && !c.opt.no_sample;
    p.slab_prior_q16 = c.opt.slab_q16 > 0 ? (uint32_t)c.opt.slab_q16 : c.ov_slab_q16;
    p.slab_pct = (uint32_t)c.opt.slab_pct;
    bool ov_slab_on = phase == 0 && half && mir16 && !c.opt.no_slab && nrows > 0 && (sampling || p.slab_prior_q16 != 0u);
    int64_t ov_slab_cap = 0;
    if (ov_slab_on) {
        ov_slab_cap = std::min<int64_t>(c.ov_tmp_cap + (int64_t)SLAB_PAD * nrows, 0xFFFF0000ll);
        if (ov_slab_cap + M >= 0xFFFFFFFFll) ov_slab_cap = std::max<int64_t>(0xFFFFFFFFll - M - 1, 0);
        if (ov_slab_cap <= (int64_t)SLAB_PAD * nrows + 1) ov_slab_on = false;
    }
    p.nsample = sampling ? 256u : 0u; p.sstep = sampling ? (uint32_t)(nrows / 256) : 1u;
    uint32_t skipped_tiers = 0;
    if (nrows > 0) {
        auto X = [&](int B, bool P) { return (size_t)256 + (size_t)(B / 64) * (P ? 3072 : (pay16 ? 2048 : 2560)); };
        const bool all_tiers = !c.ov_tiers_known || phase == 2;
        int tmax = NUM_TIERS;
        if (c.opt.tune[4] != 2 && passes == 1) {
            const uint64_t ubm = std::min<uint64_t>((uint64_t)std::max<int64_t>(c.max_row_nnz, 1) * (uint64_t)p.max_col, (uint64_t)p.Mcols);
            const int gmax = ubm <= 1 ? 1 : 64 - __builtin_clzll(2 * ubm - 1);
            tmax = gmax <= LDS_TBITS0 ? 0 : gmax - LDS_TBITS0;
            tmax = std::max(tmax, (int)p.min_tier);
            if (p.suffix) tmax = std::max(tmax, (int)p.dense_up);
        }
        o.tmax = tmax;
        const int dk = c.opt.dk >= 0 ? c.opt.dk : ((c.csr_inline && c.N > 0 && c.Z < 3 * c.N) ? 0 : 1);
        // ov_spec_ok
        const bool spec = !c.opt.ov_generic && c.opt.dk < 0 && dk == 0 && !pay && p.pay16 == 1u && c.use_ell && p.half == 1u &&
                          p.hint_mask == 1u << 31 && p.pos_mask == 0x3FFFFFFFu && p.inl == 1u && (mir16 ? 1u : 0u) == 1u &&
                          p.suffix == 0u && !p.row_order && p.qblk_log2 == 0u && (uint32_t)row_lo == 0u && (uint32_t)row_hi == (uint32_t)M && p.Mcols == (uint32_t)M &&
                          c.opt.tune[3] == 0 && c.opt.tune[4] == 0 && c.opt.tune[5] == 0 && c.opt.tune[7] == 0;
        o.dk = dk; o.spec = spec;
        // the three macros, as functions: D = ELBA_LAUNCH_D, S = ELBA_LAUNCH_S (which ignored its lds argument), DTIER = ELBA_DTIER
        auto D = [&](int B, bool G, bool P, long long grid, size_t lds, int tier, unsigned tb) {
            OldLaunch l; l.launched = true; l.B = B; l.grid = grid; l.lds = lds; l.tier = tier; l.tb = tb;
            if (spec && !G && !P) { l.spec = true; l.dk = 0; } else { l.G = G; l.P = P; l.dk = dk == 0 ? 0 : dk == 1 ? 1 : dk == 4 ? 4 : 2; }
            return l; };
        auto S = [&](int B, int TBC, long long grid, size_t, int tier, unsigned tb) {
            OldLaunch l; l.launched = true; l.B = B; l.S = true; l.TBC = TBC; l.dk = 2; l.grid = tier == 0 ? (long long)cus * c.opt.dense_wgs : grid; l.lds = (size_t)18 * (1u << tb) + 256 + (size_t)(B / 64) * 2368; l.tier = tier; l.tb = tb;
            return l; };
        auto DTIER = [&](int t, const OldLaunch &l) { if ((all_tiers || c.ov_tier_used[t]) && t <= tmax) o.tier[t] = l; else skipped_tiers |= 1u << t; };
        if (sampling) {
            if (p.suffix) o.sample = S(1024, 0, cus, (size_t)26 * 4096 + X(1024, true), 3, 12u);
            else if (pay) o.sample = D(1024, false, true, cus, (size_t)26 * 4096 + X(1024, true), 3, 12u);
            else o.sample = D(1024, false, false, cus, (size_t)18 * 4096 + X(1024, false), 3, 12u);
        }
        {
            int nb = (int)((nrows + 255) / 256);
            if (nb > cus * 4) nb = cus * 4;
            o.classify_nb = nb;
        }
        if (p.suffix) {
            DTIER(0, S(256, 9, cus * 9, (size_t)26 * 512 + X(128, true), 0, 9u));
            if (p.dense_up >= 1u) DTIER(1, S(512, 10, cus * 4, (size_t)26 * 1024 + X(256, true), 1, 10u));
            else DTIER(1, S(256, 0, cus * 4, (size_t)26 * 1024 + X(256, true), 1, 10u));
            if (p.dense_up >= 2u) DTIER(2, S(1024, 11, cus * 2, (size_t)26 * 2048 + X(512, true), 2, 11u));
            else DTIER(2, S(512, 0, cus * 2, (size_t)26 * 2048 + X(512, true), 2, 11u));
            DTIER(3, S(1024, 0, cus, (size_t)26 * 4096 + X(1024, true), 3, 12u));
        } else if (pay) {
            DTIER(0, D(128, false, true, cus * 9, (size_t)26 * 512 + X(128, true), 0, 9u));
            DTIER(1, D(256, false, true, cus * 4, (size_t)26 * 1024 + X(256, true), 1, 10u));
            DTIER(2, D(512, false, true, cus * 2, (size_t)26 * 2048 + X(512, true), 2, 11u));
            DTIER(3, D(1024, false, true, cus, (size_t)26 * 4096 + X(1024, true), 3, 12u));
        } else {
            DTIER(0, D(128, false, false, cus * 12, (size_t)18 * 512 + X(128, false), 0, 9u));
            DTIER(1, D(256, false, false, cus * 7, (size_t)18 * 1024 + X(256, false), 1, 10u));
            DTIER(2, D(512, false, false, cus * 3, (size_t)18 * 2048 + X(512, false), 2, 11u));
            DTIER(3, D(1024, false, false, cus, (size_t)18 * 4096 + X(1024, false), 3, 12u));
        }
        DTIER(4, D(256, false, false, cus, (size_t)18 * 8192 + X(256, false), 4, 13u));
        DTIER(5, D(256, true, false, spill_blocks, (size_t)256 + 4 * 2560, NUM_LDS_TIERS, 0u));
    }
    // ov_launch_finalize(c, p.half, !c.ov_tiers_known, skipped_sorts, nullptr, 0)
    {
        const bool all_sorts = !c.ov_tiers_known; const int64_t nremote = 0; const uint32_t fhalf = p.half;
        uint32_t skipped_sorts = 0;
        o.fin_slab = fhalf == 1u && mir16 && ov_slab_on;
        o.slab_fold_nb = o.fin_slab && nrows > 0 ? (nrows + 255) / 256 : 0;
        uint64_t sstride = 2;
        while (sstride < (uint64_t)M) sstride <<= 1;
        o.sstride = sstride;
        o.scan = !(M + 1 <= (1 << 17));
        o.rp_nb = o.scan ? (M + 1 + 255) / 256 : (M + 1 + RP_TILE - 1) / RP_TILE;
        if (nrows > 0) {
            int nb = (int)((nrows + 3) / 4);
            if (nb > cus * 32) nb = cus * 32;
            o.fin_nb = nb;
            skipped_sorts = 0;
            bool narrow = false;
            if (c.opt.tune[4] != 2 && std::min<uint64_t>((uint64_t)std::max<int64_t>(c.max_row_nnz, 1) * (uint64_t)std::max<int64_t>(c.max_col_nnz, 1), (uint64_t)M) <= (uint64_t)FIN_WAVE2_MAX && nremote == 0) narrow = true;
            o.narrow = narrow;
            if (!narrow && (all_sorts || c.ov_sort_used[0])) { o.bucket = true; o.bucket_nb = nrows < (int64_t)cus * 4 ? nrows : (int64_t)cus * 4; }
            else skipped_sorts |= 1u;
            if (!narrow && (all_sorts || c.ov_sort_used[1])) o.huge = true;
            else skipped_sorts |= 2u;
        }
        o.skipped_sorts = skipped_sorts;
    }
    o.gstride = gstride; o.spill_blocks = spill_blocks; o.half = half; o.slack = slack; o.ov_tmp_cap = c.ov_tmp_cap;
    o.p_half = p.half; o.pos_mask = p.pos_mask; o.hint_mask = p.hint_mask; o.suffix = p.suffix; o.inl = p.inl; o.prior_q16 = p.prior_q16; o.use_feedback = p.use_feedback;
    o.pay16 = p.pay16; o.qblk_log2 = p.qblk_log2; o.min_tier = p.min_tier; o.max_col = p.max_col; o.nsample = p.nsample; o.sstep = p.sstep; o.slab_prior_q16 = p.slab_prior_q16; o.slab_pct = p.slab_pct;
    for (int t = 0; t < 5; ++t) o.tier_limit[t] = p.tier_limit[t];
    o.row_order = p.row_order; o.pay = pay; o.mir16 = mir16; o.sampling = sampling; o.ov_slab_on = ov_slab_on; o.ov_slab_cap = ov_slab_cap; o.fb_enough = p.fb_enough; o.skipped_tiers = skipped_tiers;
    return o;
}

// ---- new against old, field by field ----------------------------------------------------------------------------------------------------------
static void same_launch(const char *what, int t, const OvPlan &p, const OvLaunch &l, bool launched, const OldLaunch &o, unsigned sample)
{
    CHECK(launched == o.launched, "%s tier %d", what, t);
    if (!launched || !o.launched) return;
    const OvTierRow &r = OV_ROWS[l.row];
    const bool spec = p.spec && !r.dense && !r.global && !r.payload;
    CHECK(r.block == o.B && l.block == o.B && l.grid == o.grid && l.lds == o.lds && r.tier == o.tier && (unsigned)r.tbits == o.tb, "%s tier %d: B %d/%d grid %d/%lld lds %zu/%zu tier %d/%d tb %d/%u", what, t, r.block, o.B, l.grid, o.grid, l.lds, o.lds, r.tier, o.tier, r.tbits, o.tb);
    CHECK(r.dense == o.S && spec == o.spec, "%s tier %d: family", what, t);
    if (r.dense) CHECK(r.tbc == o.TBC && o.dk == 2, "%s tier %d: TBC %d/%d", what, t, r.tbc, o.TBC);
    else if (spec) CHECK(o.dk == 0 && !o.G && !o.P, "%s tier %d: spec", what, t);
    else CHECK(r.global == o.G && r.payload == o.P && (p.dk == 0 || p.dk == 1 || p.dk == 4 ? p.dk : 2) == o.dk, "%s tier %d: G %d/%d P %d/%d dk %d/%d", what, t, r.global, o.G, r.payload, o.P, p.dk, o.dk);
    (void)sample;
}

static void same_as_old(const char *what, const OvInput &in)
{
    const OvPlan p = plan_ov(in);
    const OldPlan o = old_plan(in);
    const int64_t nrows = in.row_hi - in.row_lo;
    CHECK(p.nrows == nrows && p.gstride == o.gstride && p.spill_blocks == o.spill_blocks && p.slack == o.slack && p.tmp_cap == o.ov_tmp_cap && p.b_cap == o.b_cap_entries, "%s: capacities tmp %lld/%lld", what, (long long)p.tmp_cap, (long long)o.ov_tmp_cap);
    CHECK(p.half == o.p_half && p.pos_mask == o.pos_mask && p.hint_mask == o.hint_mask && p.suffix == o.suffix && p.inl == o.inl && p.row_order == o.row_order && p.hints_used == o.ov_hints_used, "%s: switches", what);
    CHECK(p.prior_q16 == o.prior_q16 && p.use_feedback == o.use_feedback && p.fb_enough == o.fb_enough && p.max_col == o.max_col, "%s: feedback", what);
    CHECK(p.pay == o.pay && (p.pay16 ? 1u : 0u) == o.pay16 && p.mir16 == o.mir16 && p.qblk_log2 == o.qblk_log2 && p.min_tier == o.min_tier, "%s: pay %d/%d pay16 %d/%u min_tier %u/%u", what, p.pay, o.pay, p.pay16, o.pay16, p.min_tier, o.min_tier);
    for (int t = 0; t < NUM_LDS_TIERS; ++t) CHECK(p.tier_limit[t] == o.tier_limit[t], "%s: tier_limit[%d] %u/%u", what, t, p.tier_limit[t], o.tier_limit[t]);
    CHECK(p.nsample == o.nsample && p.sstep == o.sstep && (p.sample.row >= 0) == o.sampling, "%s: sample", what);
    CHECK(p.slab_on == o.ov_slab_on && (!p.slab_on || p.slab_cap == o.ov_slab_cap) && p.slab_prior_q16 == o.slab_prior_q16, "%s: slabs %d/%d cap %lld/%lld", what, p.slab_on, o.ov_slab_on, (long long)p.slab_cap, (long long)o.ov_slab_cap);
    if (nrows > 0) {
        CHECK(p.tmax == o.tmax && p.dk == o.dk && p.spec == o.spec && p.classify_blocks == o.classify_nb, "%s: tmax %d/%d dk %d/%d spec %d/%d", what, p.tmax, o.tmax, p.dk, o.dk, p.spec, o.spec);
        same_launch(what, -1, p, p.sample, p.sample.row >= 0, o.sample, 1u);
    } else CHECK(p.launched == 0u && p.classify_blocks == 0 && p.sample.row < 0, "%s: nothing launched on an empty window", what);
    CHECK((nrows > 0 ? ~p.launched & 63u : 0u) == o.skipped_tiers, "%s: tiers not launched %x/%x", what, ~p.launched & 63u, o.skipped_tiers);
    for (int t = 0; t < NUM_TIERS; ++t) same_launch(what, t, p, p.tier[t], (p.launched >> t) & 1u, o.tier[t], 0u);
    const OvFinPlan &f = p.fin;
    CHECK(f.slabs == o.fin_slab && f.slab_fold_blocks == o.slab_fold_nb && f.sort_stride == o.sstride && f.scan_rowptr == o.scan && f.rowptr_blocks == o.rp_nb && f.huge_blocks == 32, "%s: finalize head", what);
    CHECK(f.row_blocks == o.fin_nb && f.narrow == o.narrow && ((f.sorts & 1u) != 0) == o.bucket && ((f.sorts & 2u) != 0) == o.huge && (nrows > 0 ? ~f.sorts & 3u : 0u) == o.skipped_sorts && (!o.bucket || f.bucket_blocks == o.bucket_nb), "%s: finalize sorts %x skipped %x/%x", what, f.sorts, ~f.sorts & 3u, o.skipped_sorts);
}

// ---- what every plan must have ----------------------------------------------------------------------------------------------------------------
static void properties(const char *what, const OvInput &in)
{
    const OvPlan p = plan_ov(in);
    const int64_t nrows = in.row_hi - in.row_lo;
    for (int t = 0; t < NUM_TIERS; ++t) {
        CHECK(p.tier[t].row >= 0 && OV_ROWS[p.tier[t].row].tier == t, "%s: tier %d has a row", what, t);
        if ((p.launched >> t) & 1u) CHECK(p.tier[t].lds <= OV_LDS_MAX && p.tier[t].grid >= 1 && p.tier[t].block % 64 == 0 && p.tier[t].block <= 1024, "%s: tier %d lds %zu grid %d", what, t, p.tier[t].lds, p.tier[t].grid);
    }
    if (p.sample.row >= 0) CHECK(p.sample.lds <= OV_LDS_MAX && OV_ROWS[p.sample.row].tier == OV_SAMPLE_TIER && nrows >= 8192 && p.sstep >= 32, "%s: sample", what);
    for (int t = 0; t < NUM_LDS_TIERS; ++t) {
        const uint32_t T = 1u << (LDS_TBITS0 + t);
        CHECK((1u << OV_ROWS[p.tier[t].row].tbits) == T && p.tier_limit[t] < T - (uint32_t)p.tier[t].block && p.tier_limit[t] < (T >> 2) * 3, "%s: tier_limit[%d] = %u", what, t, p.tier_limit[t]);
    }
    CHECK(p.tmax >= (int)p.min_tier && p.tmax >= 0, "%s: tmax %d min_tier %u", what, p.tmax, p.min_tier);
    if (nrows > 0 && p.tmax >= NUM_LDS_TIERS && (!in.hints.tiers_known || in.phase == 2 || in.hints.tier_used[NUM_LDS_TIERS])) CHECK((p.launched >> NUM_LDS_TIERS) & 1u, "%s: the HBM tier is launched", what);
    if (nrows > 0 && (!in.hints.tiers_known || in.phase == 2) && p.tmax >= NUM_LDS_TIERS) CHECK(p.launched == (1u << NUM_TIERS) - 1u, "%s: every tier", what);
    CHECK(p.launched < (1u << NUM_TIERS) && (nrows > 0 || p.launched == 0u), "%s: launched", what);
    if (p.spec) CHECK(p.half == ov_spec::half && p.inl == ov_spec::inl && p.pay16 && ov_spec::pay16 == 1u && p.mir16 && ov_spec::rec16 == 1u && p.suffix == ov_spec::suffix && p.qblk_log2 == ov_spec::qblk_log2 &&
                      p.hint_mask == ov_spec::hint_mask && p.pos_mask == ov_spec::pos_mask && !p.row_order && p.whole && in.row_lo == 0 && in.row_hi == in.M && p.ell && !p.pay && p.dk == 0 && p.family == OV_S32 && in.phase == 0, "%s: spec implies the constants", what);
    if (p.slab_on) CHECK(p.slab_cap + in.M < 0xFFFFFFFFll && p.slab_cap > (int64_t)SLAB_PAD * nrows + 1 && in.phase == 0 && p.mir16, "%s: slab bound", what);
    CHECK(p.tmp_cap >= 1024 || in.tmp_cap != 0, "%s: staging", what);
    // a second pass: every tier and both sorts, staging as large as the cursor said
    const OvInput in2 = ov_next_pass(in, p, true, 123456789ull);
    const OvPlan q = plan_ov(in2);
    CHECK(in2.pass == in.pass + 1 && q.tmp_cap == 123456789ll + p.slack && q.b_cap == (p.half ? 2 : 1) * q.tmp_cap, "%s: repeated pass capacity", what);
    if (nrows > 0) CHECK(q.launched == (1u << NUM_TIERS) - 1u && q.tmax == NUM_TIERS, "%s: repeated pass tiers %x", what, q.launched);
    if (nrows > 0 && !q.fin.narrow) CHECK(q.fin.sorts == 3u, "%s: repeated pass sorts", what);
    const OvPlan q2 = plan_ov(ov_next_pass(in, p, false, 99ull));
    CHECK(q2.tmp_cap == p.tmp_cap, "%s: a pass repeated for a missed tier keeps its staging", what);
}

static void both(const char *what, const OvInput &in) { same_as_old(what, in); properties(what, in); }

// ---- named shapes -------------------------------------------------------------------------------------------------------------------------
// a matrix built from 15 %-error reads, multiplied whole: padded columns, hints, inline partners, positions below 2^16
static OvInput reads_in()
{
    OvInput in;
    in.M = 2000; in.N = 900000; in.Z = 2100000; in.row_lo = 0; in.row_hi = in.M; in.max_row_nnz = 1800; in.max_col_nnz = 8; in.fbits = 3;
    in.pos16 = true; in.use_ell = true; in.csr_hints = true; in.csr_inline = true; in.num_cus = 256; in.free_bytes = 200ll << 30;
    return in;
}
static OvInput dense_in()
{
    OvInput in = reads_in();
    in.csr_inline = false; in.csr_hints = false; in.csr_suffix = true; in.have_row_order = true; in.N = 40000; in.Z = 1200000; in.max_col_nnz = 40; in.fbits = 6; in.max_row_nnz = 3000;
    return in;
}

static void test_named_shapes()
{
    { const OvInput in = reads_in(); both("reads whole", in);
      const OvPlan p = plan_ov(in);
      CHECK(p.spec && p.dk == 0 && p.pay16 && !p.pay && p.family == OV_S32 && p.half == 1u && p.tmax == 3 && p.launched == 15u && p.nsample == 0u && !p.slab_on, "reads whole: the reads-path instantiation");
      CHECK(p.tier[0].block == 128 && p.tier[0].grid == 256 * 12 && p.tier[0].lds == 18u * 512 + 256 + 2 * 2048 && p.tier[2].grid == 256 * 3 && p.tier[4].lds == 18u * 8192 + 256 + 4 * 2048 && p.tier[5].lds == 256u + 4 * 2560, "reads whole: pinned geometry");
      CHECK(p.tier_limit[0] == 383u && p.tier_limit[1] == 767u && p.tier_limit[2] == 1535u && p.tier_limit[3] == 3071u && p.tier_limit[4] == 6143u, "reads whole: tier limits");
      CHECK(p.gstride == 4096u && p.spill_blocks == 512 && p.tmp_cap == 1050000 + 8388672 && p.b_cap == 2 * p.tmp_cap && p.fb_enough == 65625ull, "reads whole: capacities %lld", (long long)p.tmp_cap); }
    // each option that must turn the instantiation off
    { int n = 0;
      auto off = [&](const char *what, OvInput in) { both(what, in); CHECK(!plan_ov(in).spec, "%s: general kernel", what); ++n; };
      OvInput in;
      in = reads_in(); in.opt.ov_generic = true; off("ov_generic", in);
      in = reads_in(); in.opt.no_symmetry = true; in.csr_inline = false; off("no_symmetry", in);
      in = reads_in(); in.opt.no_pay = true; off("no_pay", in);
      in = reads_in(); in.opt.tune3 = 1; off("tune3", in);
      in = reads_in(); in.opt.mir32 = true; off("mir32", in);
      in = reads_in(); in.use_ell = false; off("no_ell", in);
      in = reads_in(); in.csr_hints = false; off("no_hints", in);
      in = reads_in(); in.csr_inline = false; off("no_inline", in);
      for (int dk : {0, 1, 2, 4}) { in = reads_in(); in.opt.dk = dk; off("dk", in); CHECK(plan_ov(in).dk == dk, "dk %d", dk); }
      for (int v : {1, 2}) { in = reads_in(); in.opt.tune4 = v; off("tune4", in); }
      for (int v : {3, 6}) { in = reads_in(); in.opt.tune7 = v; off("tune7", in); CHECK(plan_ov(in).min_tier == (uint32_t)v - 1u, "tune7 %d", v); }
      in = reads_in(); in.opt.tune5 = 6; off("tune5", in); CHECK(plan_ov(in).qblk_log2 == 5u, "tune5");
      in = reads_in(); in.Z = 3 * in.N; off("Z = 3 N: two gather trips", in); CHECK(plan_ov(in).dk == 1, "dk 1");
      in = reads_in(); in.max_row_nnz = 8193; off("sequence numbers beyond 16 bits", in);
      CHECK(n == 19, "cases"); }
    // "no_sample" and "no_slab" are not among the switches the instantiation fixes
    { OvInput in = reads_in(); in.opt.no_sample = true; in.opt.no_slab = true; both("no_sample no_slab", in); CHECK(plan_ov(in).spec, "no_sample, no_slab: still the reads path"); }
    // dense
    for (int up = 0; up <= 3; ++up) {
        OvInput in = dense_in(); in.opt.dense_up = up; both("dense", in);
        const OvPlan p = plan_ov(in);
        CHECK(p.family == OV_DENSE && p.suffix == 1u && p.row_order && p.pay && !p.pay16 && !p.spec && p.pos_mask == 0xFFFFu, "dense_up %d: family", up);
        CHECK(p.tier[0].block == 256 && p.tier[0].grid == 256 * 8 && OV_ROWS[p.tier[0].row].tbc == 9 && p.tier[1].block == (up >= 1 ? 512 : 256) && OV_ROWS[p.tier[1].row].tbc == (up >= 1 ? 10 : 0) &&
              p.tier[2].block == (up >= 2 ? 1024 : 512) && OV_ROWS[p.tier[2].row].tbc == (up >= 2 ? 11 : 0) && p.tier[3].block == 1024 && OV_ROWS[p.tier[3].row].tbc == 0, "dense_up %d: rows", up);
        CHECK(p.tier[1].lds == 18u * 1024 + 256 + (size_t)(p.tier[1].block / 64) * 2368 && p.tier_limit[0] == 255u && p.tier_limit[1] == (up >= 1 ? 511u : 767u) && p.tier_limit[2] == (up >= 2 ? 1023u : 1535u), "dense_up %d: lds, limits", up);
        CHECK(p.tmax >= up, "dense_up %d: tmax", up);
        in.opt.dense_wgs = 3; CHECK(plan_ov(in).tier[0].grid == 256 * 3, "dense_wgs");
        in.have_row_order = false; CHECK(!plan_ov(in).row_order, "no row order");
        in.phase = 1; both("dense, sharded", in); CHECK(plan_ov(in).family == OV_PAY && plan_ov(in).suffix == 0u, "a dense matrix with the mirror exchange takes the general kernel");
    }
    // positions beyond 16 bits: 32-byte records, look-ups, no slabs
    { OvInput in = reads_in(); in.pos16 = false; in.csr_inline = false; both("positions beyond 16 bits", in);
      const OvPlan p = plan_ov(in); CHECK(!p.pay && !p.pay16 && !p.mir16 && !p.spec && p.family == OV_S32 && p.tier[2].lds == 18u * 2048 + 256 + 8 * 2560, "positions beyond 16 bits"); }
    // 64-bit payload: positions fit, the rows' sequence numbers do not
    { OvInput in = reads_in(); in.max_row_nnz = 9000; both("payload", in);
      const OvPlan p = plan_ov(in); CHECK(p.pay && p.family == OV_PAY && p.tier[0].grid == 256 * 9 && p.tier[1].grid == 256 * 4 && p.tier[2].grid == 256 * 2 && p.tier[3].lds == 26u * 4096 + 256 + 16 * 3072 && p.tier[4].lds == 18u * 8192 + 256 + 4 * 2560, "payload geometry"); }
    // a windowed context, phases 1 and 2
    { OvInput in = reads_in(); in.csr_inline = false; in.row_lo = 500; in.row_hi = 1500; both("window", in);
      CHECK(!plan_ov(in).spec && !plan_ov(in).whole && plan_ov(in).hint_mask == 1u << 31 && plan_ov(in).nrows == 1000, "window");
      for (int ph : {1, 2}) { in = reads_in(); in.row_lo = 500; in.row_hi = 1500; in.phase = ph; in.hints.tiers_known = true; both("phase", in);
          const OvPlan p = plan_ov(in); CHECK(p.half == 2u && p.hint_mask == 1u << 30 && !p.slab_on && !p.spec, "phase %d", ph);
          if (ph == 2) CHECK(p.launched == (1u << (p.tmax + 1)) - 1u, "phase 2 launches every tier up to tmax"); else CHECK(p.launched == 0u, "phase 1, no tier used before"); } }
    // the sampling edge, with slabs
    for (int64_t M : {8191, 8192}) { OvInput in = reads_in(); in.M = in.row_hi = M; both("sampling edge", in);
        const OvPlan p = plan_ov(in); CHECK((p.nsample == 256u) == (M == 8192) && p.slab_on == (M == 8192) && (M != 8192 || (p.sstep == 32u && p.sample.block == 1024 && p.sample.grid == 256)), "M = %lld", (long long)M);
        in.hints.prior_q16 = 20000; CHECK(plan_ov(in).nsample == 0u && !plan_ov(in).slab_on && plan_ov(in).use_feedback == 0u && plan_ov(in).prior_q16 == 20000u, "warm: no sample");
        in.hints.slab_q16 = 7; CHECK(plan_ov(in).slab_on && plan_ov(in).slab_prior_q16 == 7u, "warm: slabs from the carried ratio");
        in.opt.slab_q16 = 1 << 18; CHECK(plan_ov(in).slab_prior_q16 == 1u << 18, "forced ratio");
        in.opt.no_slab = true; CHECK(!plan_ov(in).slab_on, "no_slab"); both("sampling edge, warm", in); }
    // the min_tier edge
    for (int64_t nrows : {65535, 65536}) for (int64_t per : {1023, 1024}) { OvInput in = reads_in(); in.M = in.row_hi = nrows; in.Z = per * nrows + nrows - 1; in.N = in.Z; both("min_tier edge", in);
        CHECK(plan_ov(in).min_tier == (nrows == 65536 && per == 1024 ? 2u : 0u), "nrows %lld Z / nrows %lld", (long long)nrows, (long long)per);
        in.opt.tune4 = 1; CHECK(plan_ov(in).min_tier == 0u, "tune4 = 1"); }
    // the pay16 edge
    for (int64_t r : {8192, 8193}) { OvInput in = reads_in(); in.max_row_nnz = r; both("pay16 edge", in);      // (fbits = 3: 8192 << 3 = 65536)
        CHECK(plan_ov(in).pay16 == (r == 8192), "max_row_nnz << fbits = %lld", (long long)(r << 3)); }
    { OvInput in = reads_in(); in.fbits = 0; in.max_row_nnz = 65537; both("pay16 edge, fbits 0", in); CHECK(!plan_ov(in).pay16, "65537"); in.max_row_nnz = 65536; CHECK(plan_ov(in).pay16, "65536"); }
    // slab area + M at the 2^32 bound
    { OvInput in = reads_in(); in.M = in.row_hi = 200000000; in.Z = 8000000000ll; in.N = in.Z; in.hints.slab_q16 = 30000; in.hints.prior_q16 = 20000; in.free_bytes = 2000ll << 30; both("slab bound", in);
      const OvPlan p = plan_ov(in); CHECK(p.slab_on && p.slab_cap == 0xFFFFFFFFll - in.M - 1, "slab area clipped: %lld", (long long)p.slab_cap);
      in.M = in.row_hi = 0xFFFFFE00ll / 17 * 17; in.tmp_cap = 1 << 20; both("slab bound, no room", in); CHECK(!plan_ov(in).slab_on, "no room for slabs: tickets"); }
    // an empty window, an empty matrix, one row
    { OvInput in = reads_in(); in.row_lo = in.row_hi = 700; both("empty window", in); CHECK(plan_ov(in).launched == 0u && plan_ov(in).fin.row_blocks == 0 && plan_ov(in).fin.rowptr_blocks == 2, "empty window");
      in = reads_in(); in.M = in.N = in.Z = in.row_hi = 0; in.max_row_nnz = in.max_col_nnz = 0; both("empty matrix", in); CHECK(plan_ov(in).gstride == 2u && plan_ov(in).fin.rowptr_blocks == 1, "empty matrix");
      in = reads_in(); in.M = in.row_hi = 1; in.Z = 3; in.N = 3; in.max_row_nnz = 3; in.max_col_nnz = 1; in.csr_inline = false; both("M = 1", in);
      const OvPlan p = plan_ov(in); CHECK(p.tmax == 0 && p.launched == 1u && p.fin.narrow && p.fin.sorts == 0u && p.classify_blocks == 1 && p.fin.row_blocks == 1 && p.gstride == 2u, "M = 1: tmax %d launched %x", p.tmax, p.launched); }
    // the workspace hint, the scan path of the row pointers, known tiers
    { OvInput in = reads_in(); in.workspace_hint_bytes = 2400; both("workspace hint", in); CHECK(plan_ov(in).tmp_cap == 1024, "a hint of 75 records is raised to 1024");
      in = reads_in(); in.M = in.row_hi = 140000; both("scan", in); CHECK(plan_ov(in).fin.scan_rowptr && plan_ov(in).fin.rowptr_blocks == 547, "row pointers by the scan");
      in.M = in.row_hi = (1 << 17) - 1; CHECK(!plan_ov(in).fin.scan_rowptr && plan_ov(in).fin.rowptr_blocks == 128, "one launch up to 2^17 - 1 rows");
      in = reads_in(); in.hints.tiers_known = true; in.hints.tier_used[1] = in.hints.tier_used[5] = true; in.hints.sort_used[1] = true; in.max_col_nnz = 60; in.M = in.row_hi = 100000; both("known tiers", in);
      const OvPlan p = plan_ov(in); CHECK(p.launched == ((1u << 1) | (1u << 5)) && p.fin.sorts == 2u, "known tiers: %x sorts %x", p.launched, p.fin.sorts); }
}

// ---- random shapes ----------------------------------------------------------------------------------------------------------------------
static void test_random_shapes()
{
    std::mt19937_64 g(20250);
    auto pick = [&](std::initializer_list<int64_t> v) { return v.begin()[g() % v.size()]; };
    auto coin = [&](int one_in) { return g() % (uint64_t)one_in == 0; };
    for (int n = 0; n < 4000; ++n) {
        OvInput in;
        in.M = coin(4) ? pick({0, 1, 2, 255, 256, 8191, 8192, 65535, 65536, 131071, 131072, 140000, 4000000000ll}) : (int64_t)(g() % (coin(2) ? 100000 : 300000000));
        in.row_lo = coin(2) ? 0 : (int64_t)(g() % (uint64_t)(in.M + 1));
        in.row_hi = coin(2) ? in.M : in.row_lo + (int64_t)(g() % (uint64_t)(in.M - in.row_lo + 1));
        const int64_t nrows = in.row_hi - in.row_lo;
        in.Z = coin(3) && nrows > 0 ? nrows * pick({1, 75, 1023, 1024, 2000}) + (int64_t)(g() % (uint64_t)nrows) : (int64_t)(g() % 6000000000ull);
        in.N = coin(8) ? 0 : (coin(2) ? in.Z / 3 + (int64_t)(g() % 3) : (int64_t)(g() % 3000000000ull));
        in.max_row_nnz = coin(3) ? pick({0, 1, 2, 255, 256, 8192, 8193, 65536, 65537}) : (int64_t)(g() % 100000);
        in.max_col_nnz = coin(3) ? pick({0, 1, 2, 8, 64, 1024, 1025}) : (int64_t)(g() % 20000);
        in.fbits = (uint32_t)(g() % 8);
        in.pos16 = !coin(4); in.use_ell = !coin(4); in.csr_hints = !coin(3); in.csr_inline = in.use_ell && !coin(3); in.csr_suffix = !in.csr_inline && coin(3); in.have_row_order = coin(2);
        in.num_cus = (int)pick({256, 256, 64, 304, 1});
        OvOptions &o = in.opt;
        o.no_symmetry = coin(6); o.no_pay = coin(6); o.mir32 = coin(6); o.no_slab = coin(6); o.no_sample = coin(6); o.ov_generic = coin(8);
        o.dk = coin(3) ? (int)pick({0, 1, 2, 4}) : -1; o.dense_up = (int)(g() % 4); o.dense_wgs = 1 + (int)(g() % 16); o.slab_q16 = coin(4) ? (int)(g() % (1u << 20)) : 0; o.slab_pct = coin(4) ? 1 + (int)(g() % 1000) : 175;
        o.tune3 = coin(8); o.tune4 = coin(5) ? pick({1, 2}) : 0; o.tune5 = coin(8) ? (int64_t)(g() % 20) : 0; o.tune7 = coin(6) ? (int64_t)(g() % 9) : 0;
        in.hints.prior_q16 = coin(2) ? 0u : (uint32_t)(64 + g() % 1000000); in.hints.slab_q16 = coin(2) ? 0u : (uint32_t)(1 + g() % 1000000); in.hints.tiers_known = coin(2);
        for (int t = 0; t < NUM_TIERS; ++t) in.hints.tier_used[t] = coin(2);
        in.hints.sort_used[0] = coin(2); in.hints.sort_used[1] = coin(2);
        in.phase = coin(2) ? 0 : (int)pick({1, 2}); in.pass = coin(4) ? 2 : 1;
        in.tmp_cap = coin(2) ? 0 : (int64_t)(1024 + g() % 5000000000ull);
        in.free_bytes = (int64_t)(g() % (288ull << 30)); in.workspace_hint_bytes = coin(4) ? (int64_t)(g() % (1ull << 33)) : 0;
        char what[32]; snprintf(what, sizeof what, "random %d", n);
        both(what, in);
    }
}

// ---- the hints a call leaves ------------------------------------------------------------------------------------------------------------------
static void test_hints()
{
    std::mt19937_64 g(7);
    for (int n = 0; n < 3000; ++n) {
        OvHints old; old.prior_q16 = n % 3 == 0 ? 0u : (uint32_t)(g() % 500000); old.slab_q16 = (uint32_t)(g() % 100000);
        OvMeasured m; m.Z = (int64_t)(g() % 1000000); m.ndiag = (int64_t)(g() % 1000); m.nnz = m.ndiag + (int64_t)(g() % (n % 5 == 0 ? 100000000000ull : 1000000ull)); m.extra_nnz = n % 4 == 0 ? 5 : 0; m.whole = n % 3 != 0;
        m.fb_ub = n % 7 == 0 ? 0 : 1 + g() % 1000000; m.fb_claims = g() % (m.fb_ub + 1 + (n % 11 == 0 ? 1000000000000ull : 0ull));
        for (int t = 0; t < NUM_TIERS; ++t) m.tier_count[t] = (unsigned)(g() % 3);
        m.fin_count[0] = (unsigned)(g() % 2); m.fin_count[1] = (unsigned)(g() % 2);
        const OvHints h = ov_next_hints(old, m);
        // the old expressions (ov_finish_stats)
        uint32_t ov_slab_q16 = old.slab_q16, ov_prior_q16 = old.prior_q16;
        if (m.whole && m.Z > 0 && m.extra_nnz == 0) { const double r = 0.5 * (double)((int64_t)m.nnz - (int64_t)m.ndiag) / (double)m.Z * 65536.0; ov_slab_q16 = r < 1.0 ? 1u : (r > 4.0e9 ? 4000000000u : (uint32_t)r); }
        if (m.fb_ub > 0) { double r = 1.25 * (double)m.fb_claims / (double)m.fb_ub * 65536.0; const uint32_t q = r < 64.0 ? 64u : (r > 4.0e9 ? 4000000000u : (uint32_t)r); const uint32_t o = ov_prior_q16; if (o == 0 || q > o + o / 10 || q + o / 10 < o) ov_prior_q16 = q; }
        CHECK(h.slab_q16 == ov_slab_q16 && h.prior_q16 == ov_prior_q16 && h.tiers_known, "hints %d: slab %u/%u prior %u/%u", n, h.slab_q16, ov_slab_q16, h.prior_q16, ov_prior_q16);
        for (int t = 0; t < NUM_TIERS; ++t) CHECK(h.tier_used[t] == (m.tier_count[t] > 0), "hints %d tier %d", n, t);
        CHECK(h.sort_used[0] == (m.fin_count[0] > 0) && h.sort_used[1] == (m.fin_count[1] > 0), "hints %d sorts", n);
        CHECK(h.slab_q16 >= 1u && h.slab_q16 <= 4000000000u && (h.prior_q16 == 0u || h.prior_q16 >= 64u || h.prior_q16 == old.prior_q16) && h.prior_q16 <= 4000000000u, "hints %d: clamps", n);
    }
    // the 10 % hysteresis: a ratio within a tenth of the old one leaves it
    OvHints old; old.prior_q16 = 100000;
    OvMeasured m; m.fb_ub = 1000000;
    m.fb_claims = (unsigned long long)(1000000.0 * 105000 / 65536.0 / 1.25); CHECK(ov_next_hints(old, m).prior_q16 == 100000u, "5 %% above: kept");
    m.fb_claims = (unsigned long long)(1000000.0 * 115000 / 65536.0 / 1.25); CHECK(ov_next_hints(old, m).prior_q16 > 110000u, "15 %% above: replaced");
    m.fb_claims = (unsigned long long)(1000000.0 * 85000 / 65536.0 / 1.25); CHECK(ov_next_hints(old, m).prior_q16 < 90000u, "15 %% below: replaced");
}

// ---- the table itself ---------------------------------------------------------------------------------------------------------------------
static void test_table()
{
    for (int r = 0; r < OV_NROWS; ++r) {
        const OvTierRow &x = OV_ROWS[r];
        CHECK(x.block % 64 == 0 && x.block >= 128 && x.block <= 1024 && x.tier >= 0 && x.tier < NUM_TIERS, "row %d", r);
        CHECK(x.global == (x.tier == NUM_LDS_TIERS) && (x.global || x.tbits == LDS_TBITS0 + x.tier) && (x.tbc == 0 || (x.dense && x.tbc == x.tbits)), "row %d: table bits", r);
        CHECK(!(x.payload && x.global) && !(x.dense && (x.global || x.payload)), "row %d: template arguments", r);
        for (int pay16 = 0; pay16 < 2; ++pay16) CHECK(ov_row_lds(x, pay16) <= OV_LDS_MAX, "row %d: %zu bytes of LDS", r, ov_row_lds(x, pay16));
    }
    for (OvFamily f : {OV_DENSE, OV_PAY, OV_S32}) for (int t = 0; t < NUM_TIERS; ++t) for (int up = 0; up <= 3; ++up) CHECK(ov_row_of(f, t, up) >= 0, "family %d tier %d", (int)f, t);
}

// ---- the tier limits as literals ----------------------------------------------------------------------------------------------------------------
// tests/spgemm_edge_cases.py (TIER_LIMITS) restates these numbers and builds rows with limit - 1, limit and limit + 1 owned partners from them
static void test_tier_limit_literals()
{
    const char *redo = "the tier geometry changed: re-derive TIER_LIMITS / TIER_BLOCKS of tests/spgemm_edge_cases.py and its tier_case / guaranteed_case";
    auto same = [&](const char *what, const OvInput &in, OvFamily family, bool pay16, std::initializer_list<uint32_t> want) {
        const OvPlan p = plan_ov(in);
        CHECK(p.family == family && p.pay16 == pay16, "%s: family %d pay16 %d — %s", what, (int)p.family, (int)p.pay16, redo);
        int t = 0;
        for (uint32_t w : want) { CHECK(p.tier_limit[t] == w, "%s: tier_limit[%d] = %u, the tests hold %u — %s", what, t, p.tier_limit[t], w, redo); ++t; }
        CHECK(t == NUM_LDS_TIERS && LDS_TBITS0 == 9, "%s: %d LDS tiers from 2^%d slots — %s", what, NUM_LDS_TIERS, LDS_TBITS0, redo);
    };
    OvInput in = reads_in(); in.pos16 = false; in.csr_inline = false;
    same("s32", in, OV_S32, false, {383u, 767u, 1535u, 3071u, 6143u});
    in = reads_in(); in.opt.tune3 = 1;
    same("pay", in, OV_PAY, false, {383u, 767u, 1535u, 3071u, 6143u});
    in = reads_in();
    same("pay16", in, OV_S32, true, {383u, 767u, 1535u, 3071u, 6143u});
    in = dense_in(); in.opt.dense_up = 0;
    same("dense0", in, OV_DENSE, false, {255u, 767u, 1535u, 3071u, 6143u});
    in.opt.dense_up = 1;
    same("dense1", in, OV_DENSE, false, {255u, 511u, 1535u, 3071u, 6143u});
    in.opt.dense_up = 2;
    same("dense2", in, OV_DENSE, false, {255u, 511u, 1023u, 3071u, 6143u});
    CHECK(FIN_WAVE2_MAX == 1024u && SLAB_PAD == 16u && RP_TILE == 1024, "finalize constants — %s (widths_case, slab_case, rowptr_case)", redo);
}

int main()
{
    test_table();
    test_tier_limit_literals();
    test_named_shapes();
    test_random_shapes();
    test_hints();
    if (g_failed) { printf("%d of %d checks FAILED\n", g_failed, g_checks); return 1; }
    printf("ok %d\n", g_checks);
    return 0;
}
